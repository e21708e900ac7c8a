"""Density-matrix engine measurements -> profiles/density_matrix.json.

Input: the program of profiles/trajectory.json -- brickwork(n, 8, n) (tests/sampling_ref.py) under
create_noisemodel(50e-3, 70e-3) -- for n = 8, 10, 12, 13.

Per size, alternating call by call so that both series see the same machine state:
1. wall time of DeviceDM.reset + DeviceDM.run of the program (one deterministic evolution of rho; run
   returns after a stream synchronise, the host's planning included), and of the reset alone;
2. wall time of device.trajectory_sample of the same program at 8192 shots (the statevector trajectory
   engine, unchanged).
Then, in a loop of its own, the HIP-event time of the "dm_segment" launches, from which the share of the
measured HBM copy rate follows: a segment must move 32 x 4^n bytes.  Up to 12 qubits rho (at most 256 MiB)
sits in the Infinity Cache, so the share is then not an HBM figure.  At n = 12 also the readers: the
36-term periodic Heisenberg operator, all 66 pairs' RDMs, and 8192 shots from the diagonal.

Usage: python tools/density_matrix_profile.py [--reps 20] [--out profiles/density_matrix.json]
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

SIZES = (8, 10, 12, 13)
SHOTS = 8192
HBM_COPY_TBS = 6.29  # the measured HBM copy rate of an MI355X


def stats(ts):
    ts = np.asarray(ts) * 1e3
    q1, med, q3 = np.percentile(ts, [25, 50, 75])
    return {"median_ms": float(med), "min_ms": float(ts.min()), "q1_ms": float(q1), "q3_ms": float(q3),
            "max_ms": float(ts.max()), "reps": int(len(ts))}


def clock(fn):
    t0 = time.perf_counter()
    fn()
    return time.perf_counter() - t0


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "density_matrix.json"))
    args = ap.parse_args()

    import sampling_ref as ref
    from adaptaqc_amd import _lib
    from adaptaqc_amd.device import DeviceDM, dm_plan, trajectory_sample
    from adaptaqc_amd.noise import trajectory_program
    from adaptaqc_amd.utils.circuit_operations import create_noisemodel
    from adaptaqc_amd.utils.hamiltonians import heisenberg_hamiltonian
    from conftest import to_circuit

    nm = create_noisemodel(50e-3, 70e-3, log_fidelities=False)
    res = {"t1_ns": 50e3, "t2_ns": 70e3, "depth": 8, "shots": SHOTS, "hbm_copy_tb_per_s": HBM_COPY_TBS, "sizes": []}
    for n in SIZES:
        qc = to_circuit(n, ref.brickwork(n, 8, n))
        rows, n_events, _ = trajectory_program(qc, nm)
        plan = dm_plan(n, rows)
        dev = DeviceDM(n)
        r = {"n": n, "program_rows": int(len(rows)), "kraus_events": int(n_events), "plan": plan,
             "rho_bytes": 16 * 4 ** n, "bytes_moved": plan["segments"] * 32 * 4 ** n}

        def evolve():
            dev.reset()
            dev.run(rows)

        def shots():
            trajectory_sample(n, rows, n_events, SHOTS, 5, 0)

        evolve()  # warm-up of both engines
        shots()
        wall, wall_reset, wall_traj = [], [], []
        for _ in range(args.reps):
            wall.append(clock(evolve))
            wall_reset.append(clock(dev.reset))
            wall_traj.append(clock(shots))
        r["dm_reset_and_run_wall"] = stats(wall)
        r["dm_reset_wall"] = stats(wall_reset)
        r["trajectory_sample_wall"] = stats(wall_traj)
        r["dm_plan_host_wall"] = stats([clock(lambda: dm_plan(n, rows)) for _ in range(args.reps)])
        r["trajectory_over_dm"] = r["trajectory_sample_wall"]["median_ms"] / r["dm_reset_and_run_wall"]["median_ms"]

        _lib.timing_enable(True)
        _lib.timing_reset()
        for _ in range(args.reps):
            evolve()
        k = _lib.timing_query("dm_segment")
        _lib.timing_enable(False)
        ms = k["ms"] / args.reps
        r["dm_segment_kernels_ms"] = ms
        r["dm_segment_launches"] = int(k["launches"] // args.reps)
        r["bytes_per_s_tb"] = r["bytes_moved"] / (ms * 1e-3) / 1e12
        r["share_of_hbm_copy_rate"] = r["bytes_per_s_tb"] / HBM_COPY_TBS
        r["working_set"] = ("rho fits the 256 MiB Infinity Cache: the share is not an HBM figure" if n <= 12
                            else "rho is 1 GiB: every segment streams it from and to HBM")
        if n == 12:
            labels = list(heisenberg_hamiltonian(n, 1.0, 1.0, 1.0, periodic_bc=True))
            pairs = [(a, b) for a in range(n) for b in range(a + 1, n)]
            assert len(labels) == 36 and len(pairs) == 66
            evolve()
            dev.pauli_expect(labels), dev.pair_rdms(pairs), dev.sample(SHOTS, 5, 0)  # warm-up
            r["readers"] = {
                "pauli_expect_36_terms_wall": stats([clock(lambda: dev.pauli_expect(labels)) for _ in range(args.reps)]),
                "pair_rdms_66_pairs_wall": stats([clock(lambda: dev.pair_rdms(pairs)) for _ in range(args.reps)]),
                "sample_8192_shots_wall": stats([clock(lambda: dev.sample(SHOTS, 5, 0)) for _ in range(args.reps)]),
                "prob0_and_trace_wall": stats([clock(dev.prob0) for _ in range(args.reps)]),
            }
        dev.close()
        res["sizes"].append(r)
        print(json.dumps(r), flush=True)

    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(res, f, indent=1)


if __name__ == "__main__":
    main()
