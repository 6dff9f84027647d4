"""Time of the polynomial evaluation kernels (fnft_amd_poly_eval_device: KPolyEval + KPolyJoin) at three shapes, two
polynomials (the entries 11 and 21 of a transfer matrix) per signal, points on the unit circle as exp(i theta) rounds
them (both branches of fnft__poly_eval inside every wave):
    batch 1,  deg 2^20, n = 8,    derivative on     the segmented case
    batch 64, deg 2^16, n = 1024, derivative on
    batch 64, deg 2^16, n = 1024, derivative off
    python tests/gpu_debug/poly_eval_timing.py [--out profiles/poly_eval_timing.json] [--steps 20] [--warmup 5]
Each call is bracketed by HIP events on the launch stream (the call itself waits for the stream before it returns its
scratch); `warmup` calls of the same shape come first, the median of `steps` is reported.
Next to each time stands its fp64-VALU model: a Horner step of a complex polynomial is 4 FMA per (point, coefficient), 8
with the derivative, at the card's vector fp64 rate -- `model_ms` -- and the same with the kernel's own count, which is
twice that (the chains advance by a power of the point that is carried in two doubles, nft_kernels.h) -- `kernel_model_ms`.
`fraction_of_model` = model_ms / ms, `fraction_of_kernel_model` = kernel_model_ms / ms.
Beside the second shape: the plan's chirp-z contspec (type AB) with M = n = 1024 at batch 64, D = 2^16, 2SPLIT2_MODAL --
`contspec_ms` is the whole call (tree and chirp transform), `tree_ms` the call without a spectrum, their difference what
the M equispaced points cost; `eval_on_plan_ms` is fnft_amd_nsev_eval_device at the same n on that plan (values and
derivatives), which includes one export of the matrix per tree run.
Beside the first shape: `kernels_us`, the launches of fnft_amd_nsev_eval_device with n = 8 and the derivative on a
2SPLIT2_MODAL plan of D = 2^20 (the same polynomials' shape), each by its own event pair (Plan.set_launch_timing) --
which of the two kernels the time of the segmented case is spent in."""
import json, os, sys
ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT); sys.path.insert(0, os.path.join(ROOT, "tests"))
import numpy as np

CASES = ((1, 1 << 20, 8, True, "segmented"), (64, 1 << 16, 1024, True, ""), (64, 1 << 16, 1024, False, ""))
NPOLY = 2
# MI355X: 256 CUs x 4 SIMDs x 16 fp64 lanes per clock at 2.4 GHz (vector FMA = 2 flops: 78.6 TFLOP/s)
FP64_INSTR_PER_S = 256 * 4 * 16 * 2.4e9


def timed(torch, fn, steps, warmup):
    s = torch.cuda.current_stream()
    ts = []
    for i in range(warmup + steps):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record(s)
        fn()
        e1.record(s)
        torch.cuda.synchronize()
        if i >= warmup:
            ts.append(e0.elapsed_time(e1))
    return float(np.median(ts)), float(min(ts))


def poly_case(capi, torch, B, deg, n, deriv, steps, warmup):
    rng = np.random.default_rng(deg + n + B)
    p = torch.from_numpy(rng.standard_normal(B * NPOLY * (deg + 1)) + 1j * rng.standard_normal(B * NPOLY * (deg + 1))).cuda()
    z = torch.from_numpy(np.exp(1j * rng.uniform(0, 2 * np.pi, n))).cuda()
    val = torch.empty(B * NPOLY * n, dtype=torch.complex128, device="cuda")
    der = torch.empty(B * NPOLY * n, dtype=torch.complex128, device="cuda") if deriv else None

    def call():
        rc = capi.poly_eval_device(deg, NPOLY, B, p.data_ptr(), deg + 1, NPOLY * (deg + 1), n, z.data_ptr(), 0,
                                   val.data_ptr(), der.data_ptr() if deriv else 0)
        assert rc == 0, capi.last_error()
    ms, ms_min = timed(torch, call, steps, warmup)
    assert bool(torch.isfinite(val.real).all())
    pairs = B * NPOLY * n * (deg + 1)
    model = pairs * (8 if deriv else 4) / FP64_INSTR_PER_S * 1e3
    return dict(batch=B, deg=deg, entries=NPOLY, n=n, derivative=deriv, ms_median=ms, ms_min=ms_min, model_ms=model,
                kernel_model_ms=2 * model, fraction_of_model=model / ms, fraction_of_kernel_model=2 * model / ms,
                timed_calls=steps, warmup=warmup)


def plan_case(capi, torch, B, D, n, steps, warmup):
    T, XI = (-2.0, 2.0), (-1.0, 1.0)
    rng = np.random.default_rng(7)
    q = torch.from_numpy(0.05 * (rng.standard_normal(B * D) + 1j * rng.standard_normal(B * D))).cuda()
    plan = capi.Plan(D, n, batch=B, discretization="2SPLIT2_MODAL")
    cs = torch.empty(B * 2 * n, dtype=torch.complex128, device="cuda")
    lam = torch.from_numpy(np.linspace(XI[0], XI[1], n).astype(np.complex128)).cuda()
    out = torch.empty(B * 4 * n, dtype=torch.complex128, device="cuda")
    full = timed(torch, lambda: plan.contspec_device(q.data_ptr(), cs.data_ptr(), T, XI, contspec_type="AB"), steps, warmup)
    tree = timed(torch, lambda: plan.contspec_device(q.data_ptr(), 0, T, XI, contspec_type="AB"), steps, warmup)
    ev = timed(torch, lambda: plan.eval_device(lam.data_ptr(), n, out.data_ptr(), T, derivative=True), steps, warmup)
    assert plan.finish() == 0
    plan.close()
    return dict(contspec_ms=full[0], tree_ms=tree[0], chirp_ms=full[0] - tree[0], eval_on_plan_ms=ev[0], M=n, D=D, batch=B)


def segmented_on_plan(capi, torch, D, n):
    T = (-2.0, 2.0)
    rng = np.random.default_rng(11)
    q = torch.from_numpy(0.05 * (rng.standard_normal(D) + 1j * rng.standard_normal(D))).cuda()
    plan = capi.Plan(D, 0, batch=1, discretization="2SPLIT2_MODAL")
    lam = torch.from_numpy(np.linspace(-1.0, 1.0, n).astype(np.complex128)).cuda()
    out = torch.empty(4 * n, dtype=torch.complex128, device="cuda")
    assert plan.contspec_device(q.data_ptr(), 0, T, (-1.0, 1.0)) == 0
    for _ in range(5):     # warm: the first call also exports the matrix
        assert plan.eval_device(lam.data_ptr(), n, out.data_ptr(), T, derivative=True) == 0
    assert plan.finish() == 0
    plan.set_launch_timing(True)
    assert plan.eval_device(lam.data_ptr(), n, out.data_ptr(), T, derivative=True) == 0
    assert plan.finish() == 0
    us = [(k, 1e3 * ms) for k, ms in plan.launch_times()]
    plan.set_launch_timing(False)
    plan.close()
    return us


def main():
    args = sys.argv[1:]
    opt = lambda k, d: args[args.index(k) + 1] if k in args else d  # noqa: E731
    out_path = opt("--out", os.path.join(ROOT, "profiles", "poly_eval_timing.json"))
    steps, warmup = int(opt("--steps", 20)), int(opt("--warmup", 5))
    import torch
    from fnft_amd import build, capi
    assert torch.cuda.is_available(), "this measurement needs the GPU"
    build.build(); capi.load(); capi.silence_errors()
    rows = []
    for B, deg, n, deriv, note in CASES:
        row = poly_case(capi, torch, B, deg, n, deriv, steps, warmup)
        row["note"] = note
        if note == "segmented":
            row["kernels_us"] = segmented_on_plan(capi, torch, deg, n)
        if (B, deriv) == (64, True):
            row["plan"] = plan_case(capi, torch, B, deg, n, steps, warmup)
        rows.append(row)
        print(json.dumps(row), flush=True)
    res = dict(device=torch.cuda.get_device_name(0), build_id=build.build_id(), fp64_instr_per_s=FP64_INSTR_PER_S, rows=rows)
    os.makedirs(os.path.dirname(out_path), exist_ok=True)
    with open(out_path, "w") as f:
        json.dump(res, f, indent=1)
        f.write("\n")


if __name__ == "__main__":
    main()
