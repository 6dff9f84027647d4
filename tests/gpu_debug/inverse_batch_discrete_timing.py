"""Throughput of the batched inverse with a discrete spectrum (capi.InversePlan(K=3)) at D = 2^14, B = 64 against 64
sequential drop-in fnft_nsev_inverse calls in the same process, and the K = 0 batched call on the same continuous
spectra (the discrete stage's own cost is the difference).  Workloads: pure solitons (M = 0), b(xi) with the discrete
spectrum of tests/inverse_cases.py (b_of_xi_w_discrete, norming constants), rho with residues.  2SPLIT2_MODAL.
    python tests/gpu_debug/inverse_batch_discrete_timing.py [--out profiles/inverse_batch_discrete_timing.json]
    python tests/gpu_debug/inverse_batch_discrete_timing.py --one   # the batched calls only, two each (kernel trace)
Batched calls: one warm-up call, then device-synchronised, best of `reps`.  Drop-in: one warm-up call, then B calls."""
import json, os, sys, time
ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT); sys.path.insert(0, os.path.join(ROOT, "tests"))
import numpy as np
import torch
from fnft_amd import build, capi
import inverse_cases as IC

capi.load(); capi.silence_errors()
DISC = "2SPLIT2_MODAL"
D, B, K = 1 << 14, 64, 3


def workloads():
    xo = lambda D_, T_, M_: capi.nsev_inverse_XI(D_, T_, M_, DISC)[1]
    s = np.arange(B)
    # pure solitons: three bound states per signal, moved along the real axis, norming constants of unit modulus
    bs_sol = np.stack([1j * np.array([0.5, 1.5, 2.5]) + 0.01 * k for k in s])
    nc_sol = np.stack([np.array([-1.0, 1.0, -1.0]) * np.exp(0.1j * k) for k in s])
    sol = dict(name="pure_solitons", M=0, T=[-15.0, 15.0], XI=None, cs=None, bs=bs_sol, nc=nc_sol,
               opts={"discretization": DISC})
    # b(xi) with the discrete spectrum of b_of_xi_w_discrete (A = 3.45: K = 3), D = 2^14
    c = IC.b_cases("b_of_xi", True, "2split2_modal", 5, xo)
    assert c["D"] == D and len(c["bound_states"]) == K
    cs = np.stack([np.asarray(c["contspec"]) * (1.0 - 0.005 * k) for k in s])
    bs = np.stack([c["bound_states"] + 0.01 * k for k in s])
    nc = np.stack([c["normconsts"] * np.exp(0.1j * k) for k in s])
    bxi = dict(name="b_of_xi_discrete", M=c["M"], T=c["T"], XI=c["XI"], cs=cs, bs=bs, nc=nc,
               opts=dict(c["opts"], discretization=DISC))
    # rho (|rho| < 1 from the same b) with residues
    rho = dict(name="rho_residues", M=c["M"], T=c["T"], XI=c["XI"], cs=cs / np.sqrt(1.0 + np.abs(cs) ** 2), bs=bs,
               nc=nc * 0.5j, opts={"discretization": DISC, "discspec_type": "RESIDUES"})
    return [sol, bxi, rho]


def timed(fn, reps):
    ts = []
    for r in range(reps + 1):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        if r:
            ts.append(time.perf_counter() - t0)
    return min(ts)


def batched(w, Kp, reps):
    """ms per batched call (K = Kp; Kp = 0: the continuous part alone), q[B, D]"""
    M = w["M"]
    opts = dict(w["opts"])
    if Kp == 0:
        opts.pop("discspec_type", None)
    plan = capi.InversePlan(D, M, B, opts, K=Kp)
    dcs = None if w["cs"] is None else torch.from_numpy(np.ascontiguousarray(w["cs"]).reshape(-1)).to("cuda")
    dbs = torch.from_numpy(np.ascontiguousarray(w["bs"]).reshape(-1)).to("cuda")
    dnc = torch.from_numpy(np.ascontiguousarray(w["nc"]).reshape(-1)).to("cuda")
    dq = torch.empty(B * D, dtype=torch.complex128, device="cuda")

    def call():
        if Kp:
            rc = plan.run_device_discrete(0 if dcs is None else dcs.data_ptr(), dbs.data_ptr(), dnc.data_ptr(),
                                          dq.data_ptr(), w["XI"], w["T"], 1)
        else:
            rc = plan.run_device(dcs.data_ptr(), dq.data_ptr(), w["XI"], w["T"], 1)
        assert rc == 0, capi.last_error()
        rcf, st, _ = plan.finish()
        assert rcf == 0, (rcf, st)
    t = timed(call, reps)
    q = dq.cpu().numpy().reshape(B, D)
    ws = plan.workspace_bytes()
    plan.close()
    return t * 1e3, q, ws


def drop_in(w, b):
    cs = None if w["cs"] is None else w["cs"][b].copy()
    rc, q = capi.fnft_nsev_inverse(w["M"], cs, w["XI"], w["bs"][b], w["nc"][b], D, w["T"], 1, w["opts"])
    assert rc == 0, capi.last_error()
    return q


def one(w, reps=5):
    ms, q, ws = batched(w, K, reps)
    r = dict(workload=w["name"], D=D, M=w["M"], B=B, K=K, batched_ms=ms, workspace_bytes=ws)
    if w["M"]:
        ms0, _, _ = batched(w, 0, reps)
        r.update(continuous_only_batched_ms=ms0, discrete_stage_ms=ms - ms0)
    drop_in(w, 0)    # warm-up
    t0 = time.perf_counter()
    diff = 0.0
    for b in range(B):
        q0 = drop_in(w, b)
        diff = max(diff, float(np.max(np.abs(q[b] - q0)) / np.max(np.abs(q0))))
    seq = time.perf_counter() - t0
    r.update(sequential_ms=seq * 1e3, speedup=seq * 1e3 / ms, max_rel_diff_vs_drop_in=diff)
    return r


def main():
    ws = workloads()
    if "--one" in sys.argv:
        for w in ws:
            print(w["name"], batched(w, K, 1)[0], "ms", flush=True)
        return
    out_path = sys.argv[sys.argv.index("--out") + 1] if "--out" in sys.argv else None
    res = []
    for w in ws:
        r = one(w)
        print(json.dumps(r), flush=True)
        res.append(r)
    doc = dict(build_id=build.build_id(), device=torch.cuda.get_device_name(0), discretization=DISC, results=res)
    if out_path:
        with open(out_path, "w") as f:
            json.dump(doc, f, indent=1)


if __name__ == "__main__":
    main()
