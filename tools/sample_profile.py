"""Shot-sampling measurements -> profiles/sampling.json.

- 8192 shots of the bench's 50-qubit chi = 64 state (bench.near_product_mps): wall time of
  DeviceMPS.sample, and the HIP-event time of its two parts (the environment build "sample_env" and
  the sampler kernel "mps_sample"), i.e. with and without the environment build;
- 8192 shots of a 20-qubit brickwork statevector;
- beside each, one replay of the state's circuit: for the MPS an evaluation's replay as the bench
  runs it (reload of the cached state, one thin layer at max_chi = 64, sort); for the statevector
  reset + apply of the whole circuit;
- aqc_mps_z_all_batch on the same MPS (the existing GEMM chain closest in shape);
- the MPS sampler's share of the FP64 matrix-core peak from the analytic flop count
  8 (2 chi_l chi_r + 2 chi_r^2) per shot and site.

Usage: python tools/sample_profile.py [--shots 8192] [--reps 5] [--out profiles/sampling.json]
"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import bench  # noqa: E402


def timed(fn, reps):
    fn()
    ts = []
    for _ in range(reps):
        t0 = time.perf_counter()
        fn()
        ts.append((time.perf_counter() - t0) * 1e3)
    return {"median_ms": float(np.median(ts)), "min_ms": float(np.min(ts)), "reps": reps}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--shots", type=int, default=8192)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "sampling.json"))
    args = ap.parse_args()

    import sampling_ref as ref
    from adaptaqc_amd import _lib
    from adaptaqc_amd.circuit import device_ops
    from adaptaqc_amd.device import DeviceMPS, DeviceSV, z_all_batch
    from conftest import to_circuit

    shots, reps = args.shots, args.reps
    peak = float(getattr(bench, "FP64_PEAK_TFLOPS", 78.6))
    res = {"shots": shots, "fp64_matrix_peak_tflops": peak}

    # ---- MPS: the bench's 50-qubit chi = 64 state ------------------------------------------------
    n, chi = bench.N_QUBITS, 64
    base = DeviceMPS(n, chi, 1e-16, chi)
    base.load_aer(bench.near_product_mps(n, chi, 1000))
    work = DeviceMPS(n, chi, 1e-16, chi)
    layer = _lib.ops_array(bench.thin_layer_ops(24, 25, [0.3, -0.2, 0.5, 0.1]))

    def replay():
        work.copy_from(base)
        work.apply(layer)
        work.sort()
        work.overlap_zero()  # (waits for the queued work, as an evaluation's read-back does)

    dims = base.dims().astype(np.float64)
    flops = shots * float(np.sum(8.0 * (2.0 * dims[:-1] * dims[1:] + 2.0 * dims[1:] ** 2)))
    mps = {"n": n, "chi": chi, "analytic_flops": flops}
    mps["sample_wall"] = timed(lambda: base.sample(shots, 1), reps)
    _lib.timing_enable(True)
    _lib.timing_reset()
    for _ in range(reps):
        base.sample(shots, 1)
    env, ker = _lib.timing_query("sample_env"), _lib.timing_query("mps_sample")
    _lib.timing_reset()
    for _ in range(reps):
        z_all_batch([base])
    zall = _lib.timing_query("mps_zall")
    _lib.timing_enable(False)
    mps["env_build_ms"] = env["ms"] / max(env["launches"], 1)
    mps["sampler_kernel_ms"] = ker["ms"] / max(ker["launches"], 1)
    mps["with_env_build_ms"] = mps["env_build_ms"] + mps["sampler_kernel_ms"]
    mps["sampler_tflops"] = flops / (mps["sampler_kernel_ms"] * 1e-3) / 1e12
    mps["sampler_share_of_fp64_matrix_peak"] = mps["sampler_tflops"] / peak
    mps["z_all_batch_kernels_ms"] = zall["ms"] / max(zall["launches"], 1)
    mps["z_all_batch_tflops"] = zall["flops"] / max(zall["launches"], 1) / (mps["z_all_batch_kernels_ms"] * 1e-3) / 1e12
    mps["z_all_batch_wall"] = timed(lambda: z_all_batch([base]), reps)
    mps["replay_wall"] = timed(replay, reps)
    res["mps"] = mps

    # ---- statevector: 20-qubit brickwork ---------------------------------------------------------
    n = 20
    ops = _lib.ops_array(device_ops(to_circuit(n, ref.brickwork(n, 8, 0))))
    sv = DeviceSV(n)
    sv.apply(ops)

    def sv_replay():
        sv.reset()
        sv.apply(ops)
        sv.amp0()

    res["statevector"] = {"n": n, "gates": int(len(ops)), "sample_wall": timed(lambda: sv.sample(shots, 1), reps),
                          "replay_wall": timed(sv_replay, reps)}
    _lib.timing_enable(True)
    _lib.timing_reset()
    for _ in range(reps):
        sv.sample(shots, 1)
    k = _lib.timing_query("sv_sample")
    _lib.timing_enable(False)
    res["statevector"]["sampler_kernels_ms"] = k["ms"] / max(k["launches"], 1)

    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(res, f, indent=1)
    print(json.dumps(res))


if __name__ == "__main__":
    main()
