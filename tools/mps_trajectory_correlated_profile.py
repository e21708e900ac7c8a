"""Correlated two-qubit errors on the MPS trajectory engine -> profiles/mps_trajectory_correlated.json.

Input: brickwork(50, 4, 50) (tests/sampling_ref.py, the circuit of profiles/mps_trajectory.json) at 2048
shots and the capacity of chi_cap_for (64), with an error on cx only, under three settings:
  (i)   depolarizing_error(p, 2) on cx, under aqc_mps_traj_set_correlated 1 (the product-unitary path: one
        row on the two sites, no centre move, no SVD) and 2 (the same groups as general two-site updates);
  (ii)  depolarizing_error(p).expand(depolarizing_error(p)) on cx: two one-qubit Kraus rows per gate, each
        at the centre.  A library without correlated groups runs this one too: --baseline-only measures it
        alone, for a checkout of the parent commit on the same machine (its result goes under "baseline"
        with --baseline FILE);
  (iii) collective decay (gamma = 0.3) on cx: a general group per gate.
p = 0.01.  Per setting: the plan's counts and the wall time of device.mps_trajectory_sample (the schedule
included; it ends in a device synchronise), one warm-up call, then --reps calls; quartiles recorded.

Usage: python tools/mps_trajectory_correlated_profile.py [--reps 5] [--baseline FILE] [--baseline-only]
           [--out profiles/mps_trajectory_correlated.json]
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

N, DEPTH, SHOTS, P = 50, 4, 2048, 0.01


def stats(ts):
    ts = np.asarray(ts) * 1e3
    q1, med, q3 = np.percentile(ts, [25, 50, 75])
    return {"median_ms": float(med), "min_ms": float(ts.min()), "q1_ms": float(q1), "q3_ms": float(q3),
            "max_ms": float(ts.max()), "reps": int(len(ts))}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--baseline", default=None, help="the JSON a --baseline-only run of the parent commit wrote")
    ap.add_argument("--baseline-only", action="store_true")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "mps_trajectory_correlated.json"))
    args = ap.parse_args()

    import sampling_ref as ref
    from adaptaqc_amd import noise
    from adaptaqc_amd.device import mps_trajectory_plan, mps_trajectory_sample
    from adaptaqc_amd.mps_operations import chi_cap_for
    from conftest import to_circuit

    qc = to_circuit(N, ref.brickwork(N, DEPTH, N))
    cap = chi_cap_for(N, None)

    def cx_model(error):
        nm = noise.NoiseModel()
        nm.add_all_qubit_quantum_error(error, "cx")
        return nm

    def measure(label, error, **kw):
        rows, n_events, _ = noise.trajectory_program(qc, cx_model(error))
        plan = mps_trajectory_plan(N, rows, **kw)
        updates = plan["gate_updates"] + plan["swap_updates"] + plan["centre_moves"]

        def run():
            t0 = time.perf_counter()
            mps_trajectory_sample(N, rows, n_events, SHOTS, 5, chi_cap=cap, **kw)
            return time.perf_counter() - t0

        run()  # warm-up
        r = {"setting": label, "program_rows": int(len(rows)), "events": int(n_events), "plan": plan,
             "two_site_updates_without_groups": updates, "wall": stats([run() for _ in range(args.reps)])}
        print(json.dumps(r), flush=True)
        return r

    one = noise.depolarizing_error(P)
    res = {"n": N, "depth": DEPTH, "shots": SHOTS, "chi_cap": cap, "p": P, "settings": []}
    product = ("(ii) product of two one-qubit depolarizing errors", one.expand(one))
    if args.baseline_only:
        res["settings"].append(measure(*product))
    else:
        import trajectory2_ref as t2ref

        dep = noise.depolarizing_error(P, 2)
        res["settings"].append(measure("(i) depolarizing_error(p, 2), mode 1 (product-unitary path)", dep, correlated=1))
        res["settings"].append(measure("(i) depolarizing_error(p, 2), mode 2 (general path)", dep, correlated=2))
        res["settings"].append(measure(*product))
        res["settings"].append(measure("(iii) collective decay, gamma = 0.3 (general path)",
                                       noise.QuantumError.two_qubit(t2ref.collective_decay(0.3)), correlated=1))
        if args.baseline:
            with open(args.baseline) as f:
                res["baseline"] = json.load(f)["settings"][0]
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(res, f, indent=1)


if __name__ == "__main__":
    main()
