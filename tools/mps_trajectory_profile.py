"""MPS trajectory measurements -> profiles/mps_trajectory.json.

Input: brickwork(n, 4, n) (tests/sampling_ref.py) on 30 and 50 qubits under create_noisemodel(50e-3,
70e-3): thermal relaxation with T1 = 50 us and T2 = 70 us against the reference's instruction times
(rx / ry 100 ns, cx 300 ns on both qubits, rz virtual); 256 and 2048 shots through
SamplingSimulator(method="matrix_product_state", mps_trajectories=True), i.e. aqc_mps_traj_sample at
the capacity of chi_cap_for (64).

Per (n, shots): the plan's counts (aqc_mps_traj_plan), the wall time of the noisy run (the host's
trajectory_program and the schedule included; it ends in a device synchronise), and in a loop of its
own the HIP-event times of k_mps_kraus1 ("mps_kraus1") and of the two-site kernels that carry event
timers ("mps_theta" + "mps_svd" + "mps_split"), from which the time per two-site update of one state
follows (event time / (the plan's two-site updates x shots)).

The yardstick is the lock-step path on its own: the same circuit's noiseless program through
aqc_mps_apply_batch on 256 fresh states of the same capacity in the same process, the same three
timer families / (two-site updates x 256).  The fused chain is switched off for both event-time loops
(256 states at capacity 64 would otherwise take k_chain in the yardstick), not for the wall times.
Quartiles over the repetitions are recorded with every wall-time series.

Usage: python tools/mps_trajectory_profile.py [--reps 5] [--out profiles/mps_trajectory.json]
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

SIZES = ((30, 256), (30, 2048), (50, 256), (50, 2048))
FAMILIES = ("mps_theta", "mps_svd", "mps_split")
YARD_STATES = 256


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
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "mps_trajectory.json"))
    args = ap.parse_args()

    import sampling_ref as ref
    from adaptaqc_amd import _lib
    from adaptaqc_amd.backends.qiskit_sampling_backend import SamplingSimulator
    from adaptaqc_amd.circuit import device_ops_array
    from adaptaqc_amd.device import DeviceMPS, apply_batch, mps_trajectory_plan
    from adaptaqc_amd.mps_operations import chi_cap_for
    from adaptaqc_amd.noise import trajectory_program
    from adaptaqc_amd.utils.circuit_operations import create_noisemodel
    from conftest import to_circuit

    nm = create_noisemodel(50e-3, 70e-3, log_fidelities=False)
    res = {"t1_ns": 50e3, "t2_ns": 70e3, "depth": 4, "yardstick_states": YARD_STATES, "sizes": []}

    def two_site_ms():
        return sum(_lib.timing_query(f)["ms"] for f in FAMILIES)

    for n, shots in SIZES:
        qc = to_circuit(n, ref.brickwork(n, 4, n))
        rows, n_events, _ = trajectory_program(qc, nm)
        plan = mps_trajectory_plan(n, rows)
        updates = plan["gate_updates"] + plan["swap_updates"] + plan["centre_moves"]
        cap = chi_cap_for(n, None)
        sim = SamplingSimulator(method="matrix_product_state", seed=1, mps_trajectories=True)
        r = {"n": n, "shots": shots, "chi_cap": cap, "program_rows": int(len(rows)), "kraus_events": int(n_events),
             "plan": plan, "two_site_updates": updates,
             "updates_per_gate": updates / max(plan["gate_updates"], 1)}

        def noisy():
            return sim.run(qc, shots=shots, seed_simulator=5, noise_model=nm).result().get_counts()

        noisy()  # warm-up
        r["noisy_run_wall"] = stats([clock(noisy)[0] for _ in range(args.reps)])

        lib = _lib.lib()
        _lib.check(lib.aqc_mps_set_fused_chain(0))
        try:
            _lib.timing_enable(True)
            _lib.timing_reset()
            noisy()
            r["mps_kraus1_ms"] = _lib.timing_query("mps_kraus1")["ms"]
            r["mps_kraus1_us_per_row_launch"] = 1e3 * r["mps_kraus1_ms"] / max(_lib.timing_query("mps_kraus1")["launches"], 1)
            r["two_site_event_ms"] = two_site_ms()
            r["us_per_two_site_update"] = 1e3 * r["two_site_event_ms"] / (updates * shots)
            # the yardstick: the noiseless program, lock-step, on fresh states
            ops = device_ops_array(qc)
            gates = int(np.count_nonzero(ops["nq"] == 2))
            states = [DeviceMPS(n, cap) for _ in range(YARD_STATES)]
            apply_batch(states, [ops] * YARD_STATES)  # warm-up
            del states
            states = [DeviceMPS(n, cap) for _ in range(YARD_STATES)]
            _lib.timing_reset()
            apply_batch(states, [ops] * YARD_STATES)
            r["yardstick_two_site_updates"] = gates
            r["yardstick_two_site_event_ms"] = two_site_ms()
            r["yardstick_us_per_two_site_update"] = 1e3 * r["yardstick_two_site_event_ms"] / (gates * YARD_STATES)
            r["update_time_ratio"] = r["us_per_two_site_update"] / r["yardstick_us_per_two_site_update"]
            del states
        finally:
            _lib.timing_enable(False)
            _lib.check(lib.aqc_mps_set_fused_chain(1))
        res["sizes"].append(r)
        print(json.dumps(r), flush=True)

    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(res, f, indent=1)


if __name__ == "__main__":
    main()
