"""Cost of Richardson extrapolation on the batched nsev plans: 64 signals of 2^14 samples resident in HBM, 2SPLIT4B.
    python tests/gpu_debug/nsev_batch_richardson_timing.py [--out profiles/nsev_batch_richardson_timing.json]
Tree plan (capi.Plan, M = 2^14, BOTH) and guess plan (capi.DiscSpecPlan, 4 guesses per signal, NEWTON with 10
iterations, FULL, BOTH), each three ways: the plan with set_richardson(True), the same plan with set_richardson(False),
and 64 drop-in fnft_nsev calls with richardson_extrapolation_flag = 1 (host copies of the same signals, wall clock after
one warm-up call).  Plan calls: `steps` calls after `warmup`, each bracketed by HIP events on the launch stream; the
median is reported.  No threshold is attached to any figure; the expectation stated next to them -- the second pass
over every other sample makes a call cost about 1.5x the plain call -- had not been measured before either."""
import json, os, sys, time
ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT); sys.path.insert(0, os.path.join(ROOT, "tests"))
import numpy as np

import discspec_batch_cases as DC

DISC, D, B, M, K, NITER = "2SPLIT4B", 1 << 14, 64, 1 << 14, 4, 10
XI = [-1.4, 1.6]
OPTS = {"discretization": DISC, "bound_state_localization": "NEWTON", "bound_state_filtering": "FULL", "niter": NITER,
        "discspec_type": "BOTH"}
EXPECTATION = "about 1.5x the plain plan call (unmeasured before this file)"


def workload():
    """B chirped sech pulses (the eight of the tests, amplitudes moved a little per repetition) and their guesses"""
    q, g = [], []
    for b in range(B):
        A, c = DC.PAIRS[b % len(DC.PAIRS)]
        A += 0.002 * (b // len(DC.PAIRS)) / (B // len(DC.PAIRS))
        q.append(DC.signal(D, A, c))
        g.append(DC.guesses(A, c, K, DC.OFFSET_2SPLIT, DC.DUP_2SPLIT))
    return np.stack(q), np.stack(g)


def timed(torch, call, steps=20, warmup=4):
    s = torch.cuda.current_stream()
    ts = []
    for i in range(warmup + steps):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record(s)
        assert call(s.cuda_stream) == 0
        e1.record(s)
        torch.cuda.synchronize()
        if i >= warmup:
            ts.append(e0.elapsed_time(e1))
    return float(np.median(ts)), float(min(ts))


def main():
    import torch
    from fnft_amd import build, capi
    capi.load(); capi.silence_errors()
    out_path = sys.argv[sys.argv.index("--out") + 1] if "--out" in sys.argv else None
    q, g = workload()
    dq = torch.from_numpy(q.reshape(-1)).to("cuda")
    dg = torch.from_numpy(g.reshape(-1)).to("cuda")
    res = {}

    # ---- continuous spectrum: the tree plan
    plan = capi.Plan(D, M, B, DISC)
    dcs = torch.empty(B * 3 * M, dtype=torch.complex128, device="cuda")
    call = lambda st: plan.contspec_device(dq.data_ptr(), dcs.data_ptr(), list(DC.T), XI, contspec_type="BOTH", stream=st)
    ws0 = plan.workspace_bytes
    plain = timed(torch, call)
    assert plan.set_richardson(True) == 0
    rich = timed(torch, call)
    assert plan.finish() == 0
    ws1 = plan.workspace_bytes
    plan.close()
    out = np.zeros(3 * M, np.complex128)
    one = lambda b: capi.fnft_nsev(q[b], DC.T, M, XI, discretization=DISC, contspec_type="BOTH", richardson=True, out=out)[0]
    assert one(0) == 0
    t0 = time.perf_counter()
    for b in range(B):
        assert one(b) == 0
    seq = (time.perf_counter() - t0) * 1e3
    res["contspec"] = dict(M=M, contspec_type="BOTH", plan_richardson_ms_median=rich[0], plan_richardson_ms_min=rich[1],
                           plan_plain_ms_median=plain[0], plan_plain_ms_min=plain[1], ratio=rich[0] / plain[0],
                           dropin_richardson_ms=seq, speedup_over_dropin=seq / rich[0], workspace_bytes_plain=ws0,
                           workspace_bytes_richardson=ws1)
    print(json.dumps(res["contspec"]), flush=True)

    # ---- discrete spectrum: the guess plan
    plan = capi.DiscSpecPlan(D, K, B, OPTS)
    dbs = torch.empty(B * K, dtype=torch.complex128, device="cuda")
    dnc = torch.empty(B * 2 * K, dtype=torch.complex128, device="cuda")
    dk = torch.empty(B, dtype=torch.int64, device="cuda")
    call = lambda st: plan.run_device(dq.data_ptr(), list(DC.T), dg.data_ptr(), dbs.data_ptr(), dnc.data_ptr(),
                                      dk.data_ptr(), st)
    ws0 = plan.workspace_bytes()
    plain = timed(torch, call)
    assert plan.set_richardson(True) == 0
    rich = timed(torch, call)
    rcf, st, ko = plan.finish()
    assert rcf == 0
    ws1 = plan.workspace_bytes()
    plan.close()
    bufs = {"bs": np.zeros(K, np.complex128), "nc": np.zeros(2 * K, np.complex128)}
    found = 0

    def one_ds(b):
        rc, bs, nc, r = capi.fnft_nsev_ds(q[b], DC.T, discretization=DISC, bsloc="NEWTON", bsfilt="FULL", niter=NITER,
                                          dstype="BOTH", guesses=g[b], richardson=True, bufs=bufs)
        assert rc == 0, capi.last_error()
        return bs.size
    one_ds(0)
    t0 = time.perf_counter()
    for b in range(B):
        found += one_ds(b)
    seq = (time.perf_counter() - t0) * 1e3
    assert found == int(ko.sum())
    res["discspec"] = dict(K=K, niter=NITER, discspec_type="BOTH", plan_richardson_ms_median=rich[0],
                           plan_richardson_ms_min=rich[1], plan_plain_ms_median=plain[0], plan_plain_ms_min=plain[1],
                           ratio=rich[0] / plain[0], dropin_richardson_ms=seq, speedup_over_dropin=seq / rich[0],
                           workspace_bytes_plain=ws0, workspace_bytes_richardson=ws1, bound_states_found=found)
    print(json.dumps(res["discspec"]), flush=True)
    doc = dict(build_id=build.build_id(), device=torch.cuda.get_device_name(0), discretization=DISC, D=D, B=B,
               expectation=EXPECTATION, results=res)
    if out_path:
        with open(out_path, "w") as f:
            json.dump(doc, f, indent=1)


if __name__ == "__main__":
    main()
