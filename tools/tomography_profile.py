"""Shot-based pair tomography measurements -> profiles/tomography.json.

Input: the bench's 50-qubit chi = 64 state (bench.near_product_mps), all 1225 pairs, 8192 shots per
Pauli setting (11025 multinomial jobs, ~90 M draws).

1. wall time of each stage of the device sweep on one state: the all-pair RDM chain
   (DeviceMPS.pair_rdms), then probabilities, counts, fit and measure (device.pair_tomography, whose
   stages each end on a stream synchronisation);
2. the HIP-event time of the draw ("multinomial", from aqc_timing_query) and its rate in draws/s;
3. the exact sweep on the same state (pair_rdms + aqc_entanglement_measures), alternating with (1)
   call by call: the tomography sweep's added time is the difference of the two medians;
4. the backend's whole device sweep from a circuit (QiskitSamplingBackend(tomography="device") on a
   50-qubit depth-12 brickwork at max_chi = 64; the simulated state is cached);
5. the "circuits" route on one pair of that circuit (nine rotated 50-qubit circuits, each simulated
   and sampled in full), for scale;
6. the largest differences between the fitted and the exact concurrences over the 1225 pairs.

Every wall time ends in a device synchronise (the calls return host results).  The spread of each
series is recorded (quartiles over the repetitions) so that a difference can be read against it.

Usage: python tools/tomography_profile.py [--reps 15] [--out profiles/tomography.json]
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


def stats(ts):
    ts = np.asarray(ts) * 1e3
    q1, med, q3 = np.percentile(ts, [25, 50, 75])
    return {"median_ms": float(med), "min_ms": float(ts.min()), "q1_ms": float(q1), "q3_ms": float(q3),
            "max_ms": float(ts.max()), "reps": int(len(ts))}


def clock(fn):
    t0 = time.perf_counter()
    out = fn()
    return time.perf_counter() - t0, out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=15)
    ap.add_argument("--shots", type=int, default=8192)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "tomography.json"))
    args = ap.parse_args()

    from adaptaqc_amd import _lib
    from adaptaqc_amd.backends.qiskit_sampling_backend import QiskitSamplingBackend, SamplingSimulator
    from adaptaqc_amd.device import DeviceMPS, entanglement_measures, pair_tomography

    reps, shots = args.reps, args.shots
    n, chi = bench.N_QUBITS, 64
    pairs = [(a, b) for a in range(n) for b in range(a + 1, n)]
    aer = bench.near_product_mps(n, chi, 1000)
    base = DeviceMPS(n, chi, 1e-16, chi)
    base.load_aer(aer)
    res = {"n": n, "chi": chi, "max_bond": int(base.dims().max()), "pairs": len(pairs), "shots": shots,
           "draws": len(pairs) * 9 * shots}

    def exact():
        return entanglement_measures(base.pair_rdms(pairs), "concurrence")

    def sweep(seed, timings=None):
        t, rdms = clock(lambda: base.pair_rdms(pairs))
        if timings is not None:
            timings["rdms"] = timings.get("rdms", 0.0) + t
        return pair_tomography(rdms, shots, seed, 0, "concurrence", timings)

    c_exact = exact()  # (warm-up of every shape)
    _, c_fit = sweep(0)
    d = np.abs(c_fit - c_exact)
    res["concurrence_error_times_sqrt_shots"] = {"max": float(d.max() * np.sqrt(shots)),
                                                 "median": float(np.median(d) * np.sqrt(shots))}

    t_exact, t_sweep, stages = [], [], {}
    for r in range(reps):  # alternating: both routes see the same machine state
        t_exact.append(clock(exact)[0])
        per = {}
        t_sweep.append(clock(lambda: sweep(r + 1, per))[0])
        for k, v in per.items():
            stages.setdefault(k, []).append(v)
    res["exact_sweep_wall"] = stats(t_exact)
    res["tomography_sweep_wall"] = stats(t_sweep)
    res["stage_wall"] = {k: stats(v) for k, v in stages.items()}
    res["added_over_exact_sweep_median_ms"] = res["tomography_sweep_wall"]["median_ms"] - res["exact_sweep_wall"]["median_ms"]

    _lib.timing_enable(True)
    _lib.timing_reset()
    for r in range(reps):
        sweep(100 + r)
    k = _lib.timing_query("multinomial")
    _lib.timing_enable(False)
    res["multinomial_kernel_ms"] = k["ms"] / max(k["launches"], 1)
    res["multinomial_draws_per_s"] = res["draws"] / (res["multinomial_kernel_ms"] * 1e-3)

    # ---- through the backend, from a circuit (the state is cached after the first sweep) ----------
    # (the simulator takes gate circuits: a 50-qubit depth-12 brickwork, bonds capped at chi)
    import sampling_ref as ref
    from conftest import to_circuit

    qc = to_circuit(n, ref.brickwork(n, 12, 0))
    kwargs = {"shots": shots}
    dev = QiskitSamplingBackend(SamplingSimulator(method="matrix_product_state", seed=1, max_chi=chi), tomography="device")
    dev.pair_tomography(qc, pairs, kwargs, "concurrence")
    res["backend_circuit"] = {"depth": 12, "max_bond": int(dev.simulator._state(qc).dims().max())}
    res["backend_device_sweep_wall"] = stats([clock(lambda: dev.pair_tomography(qc, pairs, kwargs, "concurrence"))[0]
                                              for _ in range(reps)])
    cir = QiskitSamplingBackend(SamplingSimulator(method="matrix_product_state", seed=1, max_chi=chi), tomography="circuits")
    cir.pair_tomography(qc, [(3, 17)], kwargs, "concurrence")
    res["circuits_route_one_pair_wall"] = stats([clock(lambda: cir.pair_tomography(qc, [(3, 17)], kwargs, "concurrence"))[0]
                                                 for _ in range(max(3, reps // 5))])
    res["circuits_route_all_pairs_projected_ms"] = res["circuits_route_one_pair_wall"]["median_ms"] * len(pairs)

    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(res, f, indent=1)
    print(json.dumps(res))


if __name__ == "__main__":
    main()
