"""Noisy shot sampling measurements -> profiles/trajectory.json.

Input: brickwork(n, 8, seed) (tests/sampling_ref.py) under create_noisemodel(50e-3, 70e-3): thermal
relaxation with T1 = 50 us and T2 = 70 us against the reference's instruction times (rx / ry 100 ns,
cx 300 ns on both qubits, rz virtual).  8192 shots for n = 8, 10, 12, 13 (the state in LDS) and 1024
shots for n = 16 (the global workspace).

Per size, alternating call by call so that every series sees the same machine state:
1. wall time of SamplingSimulator.run with the noise model (the host's trajectory_program included);
2. wall time of the noiseless run of the same circuit (state cached, so: one aqc_sv_sample).
Then, in a loop of its own, the HIP-event time of the "sv_traj" kernel, from which trajectories/s
and program rows/s per CU follow.  Every wall time ends in a device synchronise (run
returns host counts).  Quartiles over the repetitions are recorded with every series.

Usage: python tools/trajectory_profile.py [--reps 9] [--out profiles/trajectory.json]
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

SIZES = ((8, 8192), (10, 8192), (12, 8192), (13, 8192), (16, 1024))


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
    ap.add_argument("--reps", type=int, default=9)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "trajectory.json"))
    args = ap.parse_args()

    import sampling_ref as ref
    import torch
    from adaptaqc_amd import _lib
    from adaptaqc_amd.backends.qiskit_sampling_backend import SamplingSimulator
    from adaptaqc_amd.noise import trajectory_program
    from adaptaqc_amd.utils.circuit_operations import create_noisemodel
    from conftest import to_circuit

    cus = int(torch.cuda.get_device_properties(_lib.device_index()).multi_processor_count)
    nm = create_noisemodel(50e-3, 70e-3, log_fidelities=False)
    res = {"compute_units": cus, "t1_ns": 50e3, "t2_ns": 70e3, "depth": 8, "sizes": []}
    for n, shots in SIZES:
        qc = to_circuit(n, ref.brickwork(n, 8, n))
        rows, n_events, _ = trajectory_program(qc, nm)
        in_lds = n <= 13
        reps = args.reps if in_lds else max(3, args.reps // 3)
        sim = SamplingSimulator(method="statevector", seed=1)
        r = {"n": n, "shots": shots, "program_rows": int(len(rows)), "kraus_events": int(n_events),
             "state": "lds" if in_lds else "global workspace"}

        def noisy():
            return sim.run(qc, shots=shots, seed_simulator=5, noise_model=nm).result().get_counts()

        def clean():
            return sim.run(qc, shots=shots, seed_simulator=5).result().get_counts()

        noisy()  # warm-up of every shape
        clean()
        wall, wall_clean = [], []
        for _ in range(reps):
            wall.append(clock(noisy)[0])
            wall_clean.append(clock(clean)[0])
        r["noisy_run_wall"] = stats(wall)
        r["noiseless_run_wall"] = stats(wall_clean)
        r["trajectory_program_host_wall"] = stats([clock(lambda: trajectory_program(qc, nm))[0] for _ in range(reps)])

        _lib.timing_enable(True)
        _lib.timing_reset()
        for _ in range(reps):
            noisy()
        k = _lib.timing_query("sv_traj")
        _lib.timing_enable(False)
        ms = k["ms"] / max(k["launches"], 1)
        r["sv_traj_kernel_ms"] = ms
        r["trajectories_per_s"] = shots / (ms * 1e-3)
        r["program_rows_per_s_per_cu"] = shots * len(rows) / (ms * 1e-3) / cus
        res["sizes"].append(r)
        print(json.dumps(r), flush=True)

    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(res, f, indent=1)


if __name__ == "__main__":
    main()
