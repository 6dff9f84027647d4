"""Throughput of the guess-free batched discrete spectrum (capi.DiscSpecSearchPlan) against a loop of drop-in fnft_nsev
calls on the same signals: D = 4096, fnft_nsev's default options with BOTH (2SPLIT4B, SUBSAMPLE_AND_REFINE, FULL, niter
10), K = 8, batch = 64 and 1024, signals resident in HBM (the drop-in has to be handed host copies).
    python tests/gpu_debug/nsev_batch_search_timing.py [--out profiles/nsev_batch_search_timing.json]
                                                       [--dropin-lib /path/to/other/libfnft_amd.so]
Plan call: `steps` calls after `warmup`, each bracketed by HIP events on the launch stream; the median is reported.
Stages: one more call with the plan's per-launch timers (an event pair around every launch, so their sum exceeds the
untimed call), summed by stage.  A sweep of the fixed schedule counts as idle when its Newton launch takes less than 1.5x
the last scheduled sweep's, which does no work unless a signal needs all 80 sweeps.
Drop-in: one warm-up call, then `batch` calls (contspec = NULL), wall clock, in a child process of its own -- with
--dropin-lib from another build of the library (the parent commit's: the baseline this feature must beat)."""
import json, os, subprocess, sys, time
ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT); sys.path.insert(0, os.path.join(ROOT, "tests"))
import numpy as np

import discspec_batch_cases as DC

DISC, D, K, NITER = "2SPLIT4B", 4096, 8, 10
BATCHES = (64, 1024)
OPTS = {"discretization": DISC, "bound_state_localization": "SUBSAMPLE_AND_REFINE", "bound_state_filtering": "FULL",
        "niter": NITER, "discspec_type": "BOTH"}


def workload(B):
    """B chirped sech pulses: the eight of the tests, amplitudes moved a little per repetition"""
    q = []
    for b in range(B):
        A, c = DC.PAIRS[b % len(DC.PAIRS)]
        A += 0.002 * (b // len(DC.PAIRS)) / max(1, B // len(DC.PAIRS))
        q.append(DC.signal(D, A, c))
    return np.stack(q)


def stages(launches):
    """[(kernel, ms)] of one call -> ms per stage"""
    names = [n for n, _ in launches]
    i_start = names.index("KAberthBStart")
    i_cand = names.index("KDsCandidates")
    out = dict(subsample_and_tree=sum(ms for _, ms in launches[:i_start]), start_values=launches[i_start][1],
               candidates=launches[i_cand][1])
    sweeps, cur = [], None
    for n, ms in launches[i_start + 1:i_cand]:
        if n == "KAberthBNewton":
            cur = [ms, ms]          # Newton launch, whole sweep
            sweeps.append(cur)
        else:
            cur[1] += ms
    floor = 1.5 * sweeps[79][0]
    work = [s for s in sweeps[:80] if s[0] >= floor]
    idle = [s for s in sweeps[:80] if s[0] < floor]
    out.update(sweeps_working=sum(s[1] for s in work), sweeps_working_count=len(work),
               sweeps_idle_tail=sum(s[1] for s in idle), sweeps_idle_count=len(idle),
               polish=sum(s[1] for s in sweeps[80:]))
    rest = launches[i_cand + 1:]
    out["refine"] = sum(ms for n, ms in rest if n.startswith("KDsBox") or n.startswith("KDsNewton") or n.startswith("KDsFilter"))
    out["norming"] = sum(ms for n, ms in rest if n.startswith("KDsNorm"))
    out["launches"] = len(launches)
    return out


def plan_ms(B, steps=30, warmup=5):
    import torch
    from fnft_amd import capi
    capi.load(); capi.silence_errors()
    q = workload(B)
    plan = capi.DiscSpecSearchPlan(D, K, B, OPTS)
    dq = torch.from_numpy(q.reshape(-1)).to("cuda")
    dbs = torch.empty(B * K, dtype=torch.complex128, device="cuda")
    dnc = torch.empty(B * 2 * K, dtype=torch.complex128, device="cuda")
    dk = torch.empty(B, dtype=torch.int64, device="cuda")
    s = torch.cuda.current_stream()
    ts = []
    for i in range(warmup + steps + 1):
        if i == warmup + steps:
            plan.set_launch_timing(True)
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record(s)
        rc = plan.run_device(dq.data_ptr(), list(DC.T), dbs.data_ptr(), dnc.data_ptr(), dk.data_ptr(), s.cuda_stream)
        e1.record(s)
        assert rc == 0, capi.last_error()
        torch.cuda.synchronize()
        if warmup <= i < warmup + steps:
            ts.append(e0.elapsed_time(e1))
    st = stages(plan.launches())
    plan.set_launch_timing(False)
    rcf, status, ko = plan.finish(s.cuda_stream)
    assert rcf == 0 and int(ko.sum()) == sum(DC.K_OUT) * (B // len(DC.PAIRS)), (rcf, ko[:8])
    ws, roots = plan.workspace_bytes(), plan.roots()
    plan.close()
    return dict(batched_ms_median=float(np.median(ts)), batched_ms_min=float(min(ts)), steps=steps, warmup=warmup,
                workspace_bytes=ws, roots_per_signal=roots[0], Dsub=roots[1], bound_states_found=int(ko.sum()),
                stage_ms_with_launch_timers=st)


def dropin_child(lib, B):
    """runs in a process of its own: ms of B drop-in calls with the library at `lib` (None: this build's).  Another
    build may lack symbols capi.load() binds, so only fnft_nsev and its helpers are bound here."""
    import ctypes as C
    from fnft_amd import capi
    L = C.CDLL(lib or capi.LIB_PATH)
    vp, sz = C.c_void_p, C.c_size_t
    L.fnft_nsev_default_opts.restype = capi.NsevOpts
    L.fnft_nsev_max_K.restype = sz
    L.fnft_nsev_max_K.argtypes = [sz, C.POINTER(capi.NsevOpts)]
    L.fnft_nsev.restype = C.c_int32
    L.fnft_nsev.argtypes = [sz, vp, vp, sz, vp, vp, C.POINTER(sz), vp, vp, C.c_int32, C.POINTER(capi.NsevOpts)]
    L.fnft_errwarn_setprintf.argtypes = [vp]
    L.fnft_amd_last_error.restype = C.c_char_p
    capi._lib = L
    capi.silence_errors()
    q = workload(B)
    bufs = {"bs": np.zeros(K, np.complex128), "nc": np.zeros(2 * K, np.complex128)}
    found = 0

    def call(b):
        rc, bs, nc, res = capi.fnft_nsev_ds(q[b], DC.T, discretization=DISC, bsloc="SUBSAMPLE_AND_REFINE", bsfilt="FULL",
                                            niter=NITER, dstype="BOTH", K=K, bufs=bufs)
        assert rc == 0, capi.last_error()
        return bs.size
    call(0)
    t0 = time.perf_counter()
    for b in range(B):
        found += call(b)
    ms = (time.perf_counter() - t0) * 1e3
    print(json.dumps(dict(sequential_ms=ms, bound_states_found=found)))


def main():
    if "--child-dropin" in sys.argv:
        i = sys.argv.index("--child-dropin")
        return dropin_child(sys.argv[i + 1] or None, int(sys.argv[i + 2]))
    import torch
    from fnft_amd import build
    out_path = sys.argv[sys.argv.index("--out") + 1] if "--out" in sys.argv else None
    lib = sys.argv[sys.argv.index("--dropin-lib") + 1] if "--dropin-lib" in sys.argv else ""
    res = []
    for B in BATCHES:
        r = dict(D=D, K=K, B=B, niter=NITER, discspec_type="BOTH")
        r.update(plan_ms(B))
        o = subprocess.run([sys.executable, os.path.abspath(__file__), "--child-dropin", lib, str(B)], check=True,
                           stdout=subprocess.PIPE, text=True, timeout=600).stdout
        d = json.loads(o.strip().splitlines()[-1])
        assert d["bound_states_found"] == r["bound_states_found"]
        r.update(sequential_ms=d["sequential_ms"], speedup=d["sequential_ms"] / r["batched_ms_median"])
        print(json.dumps(r), flush=True)
        res.append(r)
    doc = dict(build_id=build.build_id(), device=torch.cuda.get_device_name(0), discretization=DISC,
               drop_in_library="this build" if not lib else "another build (--dropin-lib)", results=res)
    if out_path:
        with open(out_path, "w") as f:
            json.dump(doc, f, indent=1)


if __name__ == "__main__":
    main()
