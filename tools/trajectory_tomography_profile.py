"""Noisy pair tomography measurements -> profiles/trajectory_tomography.json.

Workload: 13 qubits, brickwork(13, 8, 13) (tests/sampling_ref.py) under create_noisemodel(50e-3, 70e-3)
-- the circuit and model of profiles/trajectory.json -- all 78 pairs, 8192 shots per Pauli setting.

Series, every wall time ending in a device synchronise (each call returns host data):
1. ``device_route``: QiskitSamplingBackend(tomography="device", trajectory_tomography=True)
   .pair_tomography with the concurrence: the host's trajectory_program and readout_effects, one
   aqc_sv_traj_pair_tomo launch of 9 x 8192 trajectories, fit and measure;
2. ``trajectories_without_readout``: aqc_sv_traj_sample for 9 x 8192 shots of the same program, i.e. the
   same trajectories ending in the full-register draw instead of the pair readout;
   (1 and 2 alternate call by call so that both see the same machine state)
3. ``circuits_route``: the same sweep with tomography="circuits", nine noisy runs per pair -- the route
   a noise model had to take before; timed over ``--baseline-pairs`` pairs (default: all 78) after
   a warm-up on one pair.
Then, in a loop of its own, the HIP-event times of the "sv_traj_pair_tomo" and "sv_traj" kernels.

Usage: python tools/trajectory_tomography_profile.py [--reps 7] [--baseline-reps 2] [--out ...]
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

N, DEPTH, SHOTS = 13, 8, 8192


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
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--baseline-reps", type=int, default=2)
    ap.add_argument("--baseline-pairs", type=int, default=0, help="pairs timed on the circuits route (0: all)")
    ap.add_argument("--n", type=int, default=N)
    ap.add_argument("--shots", type=int, default=SHOTS)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "trajectory_tomography.json"))
    args = ap.parse_args()

    import sampling_ref as ref
    import torch
    from adaptaqc_amd import _lib
    from adaptaqc_amd.backends.qiskit_sampling_backend import QiskitSamplingBackend, SamplingSimulator
    from adaptaqc_amd.device import trajectory_sample
    from adaptaqc_amd.noise import trajectory_program
    from adaptaqc_amd.utils.circuit_operations import create_noisemodel
    from conftest import to_circuit

    n, shots = args.n, args.shots
    cus = int(torch.cuda.get_device_properties(_lib.device_index()).multi_processor_count)
    nm = create_noisemodel(50e-3, 70e-3, log_fidelities=False)
    qc = to_circuit(n, ref.brickwork(n, DEPTH, n))
    pairs = [(a, b) for a in range(n) for b in range(a + 1, n)]
    rows, n_events, _ = trajectory_program(qc, nm)
    kwargs = {"shots": shots, "seed_simulator": 5, "noise_model": nm}
    res = {"compute_units": cus, "n": n, "depth": DEPTH, "t1_ns": 50e3, "t2_ns": 70e3, "pairs": len(pairs),
           "shots_per_setting": shots, "trajectories": 9 * shots, "program_rows": int(len(rows)),
           "kraus_events": int(n_events)}

    dev = QiskitSamplingBackend(SamplingSimulator(method="statevector", seed=1), tomography="device",
                                trajectory_tomography=True)
    cir = QiskitSamplingBackend(SamplingSimulator(method="statevector", seed=1), tomography="circuits")

    def device_route():
        return dev.pair_tomography(qc, pairs, kwargs, "concurrence")

    def without_readout():
        return trajectory_sample(n, rows, n_events, 9 * shots, 5, 0)

    device_route()  # warm-up of every shape
    without_readout()
    wall, wall_plain = [], []
    for _ in range(args.reps):
        wall.append(clock(device_route)[0])
        wall_plain.append(clock(without_readout)[0])
    res["device_route_wall"] = stats(wall)
    res["trajectories_without_readout_wall"] = stats(wall_plain)
    print(json.dumps({k: res[k] for k in ("device_route_wall", "trajectories_without_readout_wall")}), flush=True)

    _lib.timing_enable(True)
    _lib.timing_reset()
    for _ in range(args.reps):
        device_route()
        without_readout()
    for key, name in (("sv_traj_pair_tomo_kernel_ms", "sv_traj_pair_tomo"), ("sv_traj_kernel_ms", "sv_traj")):
        k = _lib.timing_query(name)
        res[key] = k["ms"] / max(k["launches"], 1)
    _lib.timing_enable(False)
    res["readout_share_of_kernel"] = 1 - res["sv_traj_kernel_ms"] / res["sv_traj_pair_tomo_kernel_ms"]

    timed = pairs if args.baseline_pairs <= 0 else pairs[: args.baseline_pairs]
    cir.pair_tomography(qc, pairs[:1], kwargs, "concurrence")  # warm-up
    base = []
    for _ in range(args.baseline_reps):
        base.append(clock(lambda: cir.pair_tomography(qc, timed, kwargs, "concurrence"))[0])
        print(json.dumps({"circuits_route_s": base[-1], "pairs": len(timed)}), flush=True)
    res["circuits_route_pairs_timed"] = len(timed)
    res["circuits_route_wall"] = stats(base)
    per_pair = res["circuits_route_wall"]["median_ms"] / len(timed)
    res["circuits_route_ms_per_pair"] = per_pair
    res["circuits_route_all_pairs_ms"] = per_pair * len(pairs)
    res["speedup_device_over_circuits"] = per_pair * len(pairs) / res["device_route_wall"]["median_ms"]
    print(json.dumps(res), flush=True)

    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(res, f, indent=1)


if __name__ == "__main__":
    main()
