"""Throughput of the batched, device-resident inverse (capi.InversePlan) against B sequential drop-in fnft_nsev_inverse
calls in the same process, B_OF_XI (M = D) and the reflection coefficient (M = 2D), 2SPLIT2_MODAL, kappa = 1.
    python tests/gpu_debug/inverse_batch_timing.py [--out profiles/inverse_batch_timing.json]
    python tests/gpu_debug/inverse_batch_timing.py --one      # D = 2^14, B = 64, B_OF_XI only (for a kernel trace)
The batched call is timed after one warm-up call, device-synchronised, best of `reps`; the drop-in sequence after one
warm-up call (at most 64 calls are timed, the time per call is scaled to B).  Combinations with B*D > 2^22 samples are
skipped (workspace of the B_OF_XI spectral factorization: ~3.7 GB at that size)."""
import json, os, sys, time
ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT); sys.path.insert(0, os.path.join(ROOT, "tests"))
import numpy as np
import torch
from fnft_amd import build, capi

capi.load(); capi.silence_errors()
DISC, KAPPA = "2SPLIT2_MODAL", 1
MAX_SAMPLES = 1 << 22


def rows_for(cstype, D, M, B, T):
    rc, XI = capi.nsev_inverse_XI(D, T, M, DISC)
    assert rc == 0
    xi = XI[0] + (XI[1] - XI[0]) / (M - 1) * np.arange(M)
    A = np.linspace(0.1, 0.45, B)
    t0 = np.linspace(-3, 3, B)
    rows = np.stack([1j * np.exp(-2j * xi * s) * np.sin(np.pi * a) / np.cosh(np.pi * xi) for a, s in zip(A, t0)])
    if cstype == "REFLECTION_COEFFICIENT":
        rows = rows / np.sqrt(1.0 + np.abs(rows) ** 2)   # |rho| < 1, smooth
    return XI, rows


def one(cstype, D, B, reps=5, seq_max=64):
    M = D if cstype == "B_OF_XI" else 2 * D
    T = [-32.0, 32.0]
    XI, rows = rows_for(cstype, D, M, B, T)
    opts = {"discretization": DISC, "contspec_type": cstype}
    plan = capi.InversePlan(D, M, B, opts)
    dcs = torch.from_numpy(rows.reshape(-1)).to("cuda")
    dq = torch.empty(B * D, dtype=torch.complex128, device="cuda")
    ts = []
    for r in range(reps + 1):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        assert plan.run_device(dcs.data_ptr(), dq.data_ptr(), XI, T, KAPPA) == 0, capi.last_error()
        rc, st, _ = plan.finish()
        torch.cuda.synchronize()
        if r:
            ts.append(time.perf_counter() - t0)
        assert rc == 0, (rc, st)
    q = dq.cpu().numpy().reshape(B, D)
    ws = plan.workspace_bytes()
    plan.close()
    nseq = min(B, seq_max)
    drop_in(M, rows[0], XI, D, T, opts)    # warm-up
    t0 = time.perf_counter()
    diff = 0.0
    for b in range(nseq):
        q0 = drop_in(M, rows[b], XI, D, T, opts)
        diff = max(diff, float(np.max(np.abs(q[b] - q0)) / np.max(np.abs(q0))))
    seq = (time.perf_counter() - t0) / nseq * B
    bat = min(ts)
    return dict(cstype=cstype, D=D, M=M, B=B, batched_ms=bat * 1e3, sequential_ms=seq * 1e3, seq_calls_timed=nseq,
                speedup=seq / bat, batched_Msamples_per_s=B * D / bat / 1e6, max_rel_diff_vs_drop_in=diff,
                workspace_bytes=ws)


def drop_in(M, cs, XI, D, T, opts):
    rc, q = capi.fnft_nsev_inverse(M, cs.copy(), XI, None, None, D, T, KAPPA, opts)
    assert rc == 0, capi.last_error()
    return q


def main():
    if "--one" in sys.argv:
        print(json.dumps(one("B_OF_XI", 1 << 14, 64, reps=2, seq_max=4)))
        return
    out_path = sys.argv[sys.argv.index("--out") + 1] if "--out" in sys.argv else None
    res = []
    for cstype in ("B_OF_XI", "REFLECTION_COEFFICIENT"):
        for log2D in (10, 12, 14, 16):
            for B in (1, 8, 64, 256):
                D = 1 << log2D
                if B * D > MAX_SAMPLES:
                    res.append(dict(cstype=cstype, D=D, B=B, skipped="B*D > 2^22 samples"))
                    continue
                r = one(cstype, D, B)
                print(json.dumps(r), flush=True)
                res.append(r)
    doc = dict(build_id=build.build_id(), device=torch.cuda.get_device_name(0), discretization=DISC, kappa=KAPPA,
               results=res)
    if out_path:
        with open(out_path, "w") as f:
            json.dump(doc, f, indent=1)


if __name__ == "__main__":
    main()
