"""Noisy pair tomography on the MPS engine -> profiles/mps_trajectory_tomography.json.

Workload: 50 qubits, brickwork(50, 4, 50) (tests/sampling_ref.py) under create_noisemodel(50e-3, 70e-3)
-- the circuit and model of profiles/mps_trajectory.json -- all 1225 pairs.  The shot count per Pauli
setting is a power of two chosen from a calibration call at ``--calibrate`` shots so that one sweep of
the device route takes about ``--target-s`` seconds (``--shots`` overrides it); it is recorded.

Series, every wall time ending in a device synchronise (each call returns host data):
1. ``device_route``: QiskitSamplingBackend(SamplingSimulator(method="matrix_product_state",
   mps_trajectories=True), tomography="device", trajectory_tomography=True).pair_tomography with the
   concurrence: the host's trajectory_program and readout_effects, aqc_mps_traj_pair_tomo over 9 x shots
   trajectories, fit and measure;
2. ``trajectories_without_readout``: aqc_mps_traj_sample for 9 x shots shots of the same program at the
   same capacity: the same trajectories ending in the measurement sweep instead of the pair readout
   (in larger batches: the readout's workspace does not count against them);
   (1 and 2 alternate call by call so that both see the same machine state)
3. ``circuits_route``: tomography="circuits", nine noisy MPS runs per pair, timed on ``--baseline-pairs``
   pairs and SCALED to 1225 (labelled so).
Then, in a call of its own, the HIP-event times of the RDM sweep ("rdm_env" + "rdm_chain") and of
k_mps_traj_pair_draw ("mps_traj_pair_draw"), in total and per sweep of a readout sub-batch, and of the
two-site kernels and k_mps_kraus1 in total.

Usage: python tools/mps_trajectory_tomography_profile.py [--reps 3] [--shots N] [--out ...]
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

N, DEPTH = 50, 4
EVOLVE = ("mps_theta", "mps_svd", "mps_split", "mps_kraus1")
RDM = ("rdm_env", "rdm_chain")


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
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--n", type=int, default=N)
    ap.add_argument("--shots", type=int, default=0, help="shots per setting (0: from the calibration call)")
    ap.add_argument("--calibrate", type=int, default=8)
    ap.add_argument("--target-s", type=float, default=10.0)
    ap.add_argument("--baseline-pairs", type=int, default=3)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "mps_trajectory_tomography.json"))
    args = ap.parse_args()

    import sampling_ref as ref
    from adaptaqc_amd import _lib
    from adaptaqc_amd.backends.qiskit_sampling_backend import QiskitSamplingBackend, SamplingSimulator
    from adaptaqc_amd.device import mps_trajectory_plan, mps_trajectory_sample
    from adaptaqc_amd.mps_operations import chi_cap_for
    from adaptaqc_amd.noise import trajectory_program
    from adaptaqc_amd.utils.circuit_operations import create_noisemodel
    from conftest import to_circuit

    n = args.n
    nm = create_noisemodel(50e-3, 70e-3, log_fidelities=False)
    qc = to_circuit(n, ref.brickwork(n, DEPTH, n))
    pairs = [(a, b) for a in range(n) for b in range(a + 1, n)]
    rows, n_events, _ = trajectory_program(qc, nm)
    cap = chi_cap_for(n, None)
    plan = mps_trajectory_plan(n, rows, measure=False)

    def simulator():
        return SamplingSimulator(method="matrix_product_state", seed=1, mps_trajectories=True)

    dev = QiskitSamplingBackend(simulator(), tomography="device", trajectory_tomography=True)
    cir = QiskitSamplingBackend(simulator(), tomography="circuits")

    def device_route(shots):
        return dev.pair_tomography(qc, pairs, {"shots": shots, "seed_simulator": 5, "noise_model": nm}, "concurrence")

    def without_readout(shots):
        return mps_trajectory_sample(n, rows, n_events, 9 * shots, 5, 0, chi_cap=cap)

    device_route(args.calibrate)  # warm-up of every shape
    without_readout(args.calibrate)
    shots = args.shots
    calibration = None
    if shots <= 0:
        calibration = clock(lambda: device_route(args.calibrate))[0]
        shots = args.calibrate
        while 2 * shots * calibration / args.calibrate <= args.target_s:
            shots *= 2
    res = {"n": n, "depth": DEPTH, "t1_ns": 50e3, "t2_ns": 70e3, "pairs": len(pairs), "chi_cap": cap,
           "shots_per_setting": shots, "trajectories": 9 * shots, "program_rows": int(len(rows)),
           "kraus_events": int(n_events), "plan_without_measurement_sweep": plan,
           "calibration": None if calibration is None else {"shots_per_setting": args.calibrate, "wall_s": calibration}}
    print(json.dumps(res), flush=True)

    wall, wall_plain = [], []
    for _ in range(args.reps):
        wall.append(clock(lambda: device_route(shots))[0])
        wall_plain.append(clock(lambda: without_readout(shots))[0])
        print(json.dumps({"device_route_s": wall[-1], "trajectories_without_readout_s": wall_plain[-1]}), flush=True)
    res["device_route_wall"] = stats(wall)
    res["trajectories_without_readout_wall"] = stats(wall_plain)
    res["device_route_ms_per_trajectory"] = res["device_route_wall"]["median_ms"] / (9 * shots)
    res["readout_share_of_wall"] = 1 - res["trajectories_without_readout_wall"]["median_ms"] / res["device_route_wall"]["median_ms"]

    _lib.timing_enable(True)
    _lib.timing_reset()
    device_route(shots)
    q = {name: _lib.timing_query(name) for name in EVOLVE + RDM + ("mps_traj_pair_draw",)}
    _lib.timing_enable(False)
    sweeps = max(q["mps_traj_pair_draw"]["launches"], 1)  # one launch per RDM sweep of a readout sub-batch
    res["readout_sweeps"] = sweeps
    res["states_per_sweep"] = 9 * shots / sweeps
    res["rdm_sweep_event_ms_total"] = sum(q[f]["ms"] for f in RDM)
    res["pair_draw_event_ms_total"] = q["mps_traj_pair_draw"]["ms"]
    res["evolve_event_ms_total"] = sum(q[f]["ms"] for f in EVOLVE)
    res["rdm_sweep_event_ms_per_sweep"] = res["rdm_sweep_event_ms_total"] / sweeps
    res["pair_draw_event_ms_per_sweep"] = res["pair_draw_event_ms_total"] / sweeps
    readout = res["rdm_sweep_event_ms_total"] + res["pair_draw_event_ms_total"]
    res["readout_share_of_event_time"] = readout / (readout + res["evolve_event_ms_total"])

    timed = pairs[: args.baseline_pairs]
    kwargs = {"shots": shots, "seed_simulator": 5, "noise_model": nm}
    cir.pair_tomography(qc, timed[:1], kwargs, "concurrence")  # warm-up
    base = clock(lambda: cir.pair_tomography(qc, timed, kwargs, "concurrence"))[0]
    res["circuits_route_pairs_timed"] = len(timed)
    res["circuits_route_wall_s"] = base
    res["circuits_route_ms_per_pair"] = 1e3 * base / len(timed)
    res["circuits_route_all_pairs_ms_scaled"] = res["circuits_route_ms_per_pair"] * len(pairs)
    res["speedup_device_over_circuits_scaled"] = res["circuits_route_all_pairs_ms_scaled"] / res["device_route_wall"]["median_ms"]
    print(json.dumps(res), flush=True)

    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(res, f, indent=1)


if __name__ == "__main__":
    main()
