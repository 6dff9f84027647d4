"""Throughput of the slow-discretization plan (capi.SlowPlan): all seven schemes at (B, D, M) = (1, 4096, 4096),
(64, 4096, 1024) and (1, 2^16, 16), contspec_type BOTH, no Richardson pass.
    python tests/gpu_debug/nsev_slow_timing.py [--out profiles/nsev_slow_timing.json] [--steps 20] [--warmup 3]
Plan call: the plan is created once; `steps` calls after `warmup`, each bracketed by HIP events on the launch stream and
followed by a synchronise; the median is reported as ms per call and as steps per second, B * M * D_eff / t with D_eff =
D times the scheme's upsampling factor.  `fp64_peak_fraction` is steps per second times the scatter kernel's fp64
instructions per step (FP64_PER_STEP, counted from its ISA with tests/gpu_debug/isa_summary.py: the loop body of the
variant the case runs, an FMA counted as one instruction) over the vector fp64 instruction rate of the card.
Comparisons, measured in the same run, for BO and CF4_2 (the two schemes the other paths know):
  (a) what the parent commit offers for these numbers on the device, host pointers throughout, ONE signal, times B:
      seam_ms -- the fnft__nse_scatter_matrix seam with K = M alone, on samples that are already preprocessed;
      seam_with_resample_ms -- the same plus, for CF4_2, the two fnft__misc_resample calls that make those samples (the
      plan's call includes its resampling, so this is the like-for-like figure); wall clock, median of three rounds
      after a warm-up round;
  (b) cpu_ms: the CPU oracle's orc_nse_scatter_matrix on one core for one signal, times B (measured at min(M, 256) grid
      points and scaled to M: its cost is linear in M)."""
import json, os, sys, time
ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT); sys.path.insert(0, os.path.join(ROOT, "tests"))
import numpy as np

import slow_cases as SC

CASES = ((1, 4096, 4096), (64, 4096, 1024), (1, 1 << 16, 16))
# fp64 vector instructions (v_*_f64: arithmetic, compares and conversions; an FMA is one) a wave issues per step of
# D_eff in the scatter kernel's loop, counted in the ISA of hip_kernels_slow.hip (hipcc -S) along the path these cases
# run: the full 2x2 product (every chunk but a signal's first), kappa = +1 so that ks < 0 (the sincos branch of the
# real-ks variant; the expm1 branch is skipped by the whole wave).  Real-ks loop: 85 (l, ks, sqrt, argument reduction)
# + 17 + 36 (sincos, s/k) + 46 (U and the product) = 184.  The other loops have no branch a wave skips, so their count
# is the loop's total less the vector form of the product (20 per push): complex CF 457 - 20, ES4 474 - 20 per grid
# point = three steps of D_eff, TES4 569 - 60 per grid point = three steps.
FP64_PER_STEP = {"BO": 184, "CF4_2": 184, "CF4_3": 184, "CF5_3": 437, "CF6_4": 437, "ES4": 454 / 3.0, "TES4": 509 / 3.0}
# MI355X: 256 CUs x 4 SIMDs x 16 fp64 lanes per clock at 2.4 GHz (vector FMA = 2 flops: 78.6 TFLOP/s)
FP64_INSTR_PER_S = 256 * 4 * 16 * 2.4e9


def plan_ms(capi, disc, B, D, M, steps, warmup):
    import torch
    q = np.stack([SC.signal(D, 1, v % 8) for v in range(B)])
    plan = capi.SlowPlan(D, M, B, {"discretization": disc, "contspec_type": "BOTH"})
    dq = torch.from_numpy(q).cuda()
    out = torch.empty((B, 3 * M), dtype=torch.complex128, device="cuda")
    s = torch.cuda.current_stream()
    ts = []
    for i in range(warmup + steps):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record(s)
        plan(dq, SC.T_FOC, SC.XI, 1, out=out, stream=s)
        e1.record(s)
        torch.cuda.synchronize()
        if i >= warmup:
            ts.append(e0.elapsed_time(e1))
    rc, st, _ = plan.finish()
    assert rc == 0 and np.isfinite(out.cpu().numpy()).all()
    ws = plan.workspace_bytes
    plan.close()
    return float(np.median(ts)), float(min(ts)), ws


def preprocessed(capi, disc, q, eps_t):
    """The samples the scatterer seam takes: q itself (BO), or the two resampled copies weighted (CF4_2)."""
    if disc == "BO":
        return q
    s = np.sqrt(3.0) / 6.0
    _, q1 = capi.misc_resample(q, eps_t, -eps_t * s)
    _, q2 = capi.misc_resample(q, eps_t, eps_t * s)
    qp = np.empty(2 * q.size, np.complex128)
    qp[0::2] = (0.25 + s) * q1 + (0.25 - s) * q2
    qp[1::2] = (0.25 - s) * q1 + (0.25 + s) * q2
    return qp


def seam_ms(capi, disc, D, M, with_resample):
    """One signal through the host-pointer seams, wall clock, median of three rounds after a warm-up round:
    fnft__nse_scatter_matrix with K = M, and with `with_resample` also what produces its samples (for CF4_2 the two
    fnft__misc_resample calls and the weighting; nothing for BO)."""
    xi = (SC.XI[0] + (SC.XI[1] - SC.XI[0]) / (M - 1) * np.arange(M)).astype(np.complex128)
    q = SC.signal(D, 1)
    eps_t = (SC.T_FOC[1] - SC.T_FOC[0]) / (D - 1)
    qp = preprocessed(capi, disc, q, eps_t)
    ts = []
    for i in range(4):
        t0 = time.perf_counter()
        if with_resample:
            qp = preprocessed(capi, disc, q, eps_t)
        rc, _ = capi.nse_scatter_matrix(qp, eps_t, 1, xi, derivative=False, discretization=disc)
        if i:
            ts.append((time.perf_counter() - t0) * 1e3)
        assert rc == 0
    return float(np.median(ts))


def cpu_ms(capi, disc, D, M):
    import ctypes as C
    from oracle import load_oracle
    orc = load_oracle()
    eps_t = (SC.T_FOC[1] - SC.T_FOC[0]) / (D - 1)
    qp = preprocessed(capi, disc, SC.signal(D, 1), eps_t)
    Mc = min(M, 256)
    xi = (SC.XI[0] + (SC.XI[1] - SC.XI[0]) / (M - 1) * np.arange(Mc)).astype(np.complex128)
    out = np.zeros((Mc, 8), np.complex128)
    f = orc.lib.orc_nse_scatter_matrix
    f.argtypes = [C.c_size_t, C.c_void_p, C.c_double, C.c_int, C.c_size_t, C.c_void_p, C.c_void_p, C.c_int, C.c_int]
    t0 = time.perf_counter()
    rc = f(qp.size, qp.ctypes.data, float(eps_t), 1, Mc, xi.ctypes.data, out.ctypes.data, 1 if disc == "BO" else 2, 0)
    dt = (time.perf_counter() - t0) * 1e3
    assert rc == 0
    return dt * M / Mc


def main():
    args = sys.argv[1:]
    opt = lambda k, d: args[args.index(k) + 1] if k in args else d  # noqa: E731
    out_path = opt("--out", os.path.join(ROOT, "profiles", "nsev_slow_timing.json"))
    steps, warmup = int(opt("--steps", 20)), int(opt("--warmup", 3))
    import torch
    from fnft_amd import build, capi
    assert torch.cuda.is_available(), "this measurement needs the GPU"
    build.build(); capi.load(); capi.silence_errors()
    rows = []
    for B, D, M in CASES:
        for disc in SC.DISCS:
            ms, ms_min, ws = plan_ms(capi, disc, B, D, M, steps, warmup)
            n = B * M * D * capi.SLOW_UPSAMPLING[disc]
            row = dict(discretization=disc, B=B, D=D, M=M, chunks=capi.slow_plan_chunks(D, M, B)[1], ms_median=ms,
                       ms_min=ms_min, steps_per_s=n / (ms * 1e-3), workspace_bytes=ws, timed_calls=steps, warmup=warmup)
            if FP64_PER_STEP[disc] is not None:
                row["fp64_peak_fraction"] = row["steps_per_s"] * FP64_PER_STEP[disc] / FP64_INSTR_PER_S
            if disc in ("BO", "CF4_2"):
                row["seam_ms"] = seam_ms(capi, disc, D, M, False) * B
                row["seam_with_resample_ms"] = seam_ms(capi, disc, D, M, True) * B
                row["cpu_ms"] = cpu_ms(capi, disc, D, M) * B
                row["speedup_vs_seam"] = row["seam_ms"] / ms
                row["speedup_vs_seam_with_resample"] = row["seam_with_resample_ms"] / ms
                row["speedup_vs_cpu"] = row["cpu_ms"] / ms
            rows.append(row)
            print(json.dumps(row), flush=True)
    res = dict(device=torch.cuda.get_device_name(0), build_id=build.build_id(), fp64_per_step=FP64_PER_STEP,
               fp64_instr_per_s=FP64_INSTR_PER_S, rows=rows)
    os.makedirs(os.path.dirname(out_path), exist_ok=True)
    with open(out_path, "w") as f:
        json.dump(res, f, indent=1)
        f.write("\n")


if __name__ == "__main__":
    main()
