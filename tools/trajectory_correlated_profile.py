"""Correlated two-qubit errors on the trajectory sampler -> profiles/trajectory_correlated.json.

Input: the workload of tools/trajectory_profile.py at 13 qubits -- brickwork(13, 8, 13)
(tests/sampling_ref.py), 8192 shots -- under three models that differ in the error on cx only; every
other instruction carries create_noisemodel(50e-3, 70e-3)'s thermal relaxation:
  product     the product of two thermal relaxations (create_noisemodel itself: one-qubit Kraus rows only)
  depolarize  depolarizing_error(0.01, 2): groups of 16, weights independent of the state
  decay       collective decay, K0 = diag(1, 1, 1, sqrt(1 - g)), K1 = sqrt(g) |00><11|, g = 0.3: groups of
              2, weights from the 4x4 reduced density matrix

1. The old path must not pay for the group code: ``product`` on a checkout of the parent commit
   (--parent-root, with its own built library) and on this tree, in fresh processes that alternate.
   A repeat is one process: a warm-up, then ``--calls`` timed SamplingSimulator.run calls, of which it
   reports the median.  Recorded: every repeat, the median over the repeats and their spread (max - min).
2. ``depolarize`` and ``decay`` on this tree, the same way: what the state-independent path saves over
   the RDM pass.
Beside the wall time of ``run`` every repeat records the mean HIP-event time of the sv_traj kernel.

Usage: python tools/trajectory_correlated_profile.py [--parent-root DIR] [--repeats 5] [--calls 9]
       [--out profiles/trajectory_correlated.json]
"""
import argparse
import json
import os
import subprocess
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
N, DEPTH, SHOTS = 13, 8, 8192


def worker(root, variant, calls):
    """One repeat, in this process: prints one JSON line."""
    sys.path.insert(0, root)
    sys.path.insert(0, os.path.join(root, "tests"))
    import sampling_ref as ref
    from adaptaqc_amd import _lib, noise
    from adaptaqc_amd.backends.qiskit_sampling_backend import SamplingSimulator
    from adaptaqc_amd.utils import circuit_operations as co
    from conftest import to_circuit

    nm = co.create_noisemodel(50e-3, 70e-3, log_fidelities=False)
    if variant != "product":
        if variant == "depolarize":
            cx = noise.depolarizing_error(0.01, 2)
        else:
            k1 = np.zeros((4, 4))
            k1[0, 3] = np.sqrt(0.3)
            cx = noise.QuantumError.two_qubit([np.diag([1.0, 1.0, 1.0, np.sqrt(0.7)]), k1])
        table = nm.instructions()
        nm = noise.NoiseModel()
        for name, error in table.items():
            nm.add_all_qubit_quantum_error(cx if name == "cx" else error, name)
    qc = to_circuit(N, ref.brickwork(N, DEPTH, N))
    rows, n_events, _ = noise.trajectory_program(qc, nm)
    sim = SamplingSimulator(method="statevector", seed=1)

    def run():
        return sim.run(qc, shots=SHOTS, seed_simulator=5, noise_model=nm).result().get_counts()

    first = run()  # warm-up
    wall = []
    for _ in range(calls):
        t0 = time.perf_counter()
        run()
        wall.append((time.perf_counter() - t0) * 1e3)
    _lib.timing_enable(True)
    _lib.timing_reset()
    for _ in range(3):
        run()
    k = _lib.timing_query("sv_traj")
    _lib.timing_enable(False)
    print(json.dumps({"variant": variant, "program_rows": int(len(rows)), "events": int(n_events),
                      "run_wall_ms": wall, "run_wall_median_ms": float(np.median(wall)),
                      "sv_traj_kernel_ms": k["ms"] / max(k["launches"], 1),
                      "outcomes_seen": len(first), "most_frequent": max(first, key=first.get)}), flush=True)


def repeat(root, variant, calls):
    out = subprocess.run([sys.executable, os.path.abspath(__file__), "--worker", variant, "--root", root,
                          "--calls", str(calls)], capture_output=True, text=True, timeout=300)
    if out.returncode != 0:
        raise RuntimeError(f"{variant} in {root} ended with status {out.returncode}:\n{out.stderr[-2000:]}")
    return json.loads(out.stdout.strip().splitlines()[-1])


def summary(commit, reps):
    med = [r["run_wall_median_ms"] for r in reps]
    ker = [r["sv_traj_kernel_ms"] for r in reps]
    return {"commit": commit, "repeats": reps, "median_ms": float(np.median(med)),
            "spread_ms": float(max(med) - min(med)), "kernel_median_ms": float(np.median(ker)),
            "kernel_spread_ms": float(max(ker) - min(ker))}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--parent-root", default=None, help="a built checkout of the parent commit")
    ap.add_argument("--parent-commit", default="parent")
    ap.add_argument("--commit", default="this change")
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--calls", type=int, default=9)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "trajectory_correlated.json"))
    ap.add_argument("--worker", default=None)
    ap.add_argument("--root", default=ROOT)
    args = ap.parse_args()
    if args.worker:
        worker(os.path.abspath(args.root), args.worker, args.calls)
        return

    res = {"n": N, "depth": DEPTH, "shots": SHOTS, "calls_per_repeat": args.calls,
           "what": "wall time of SamplingSimulator.run under a noise model; a repeat is one fresh process"}
    sides = {"this": (ROOT, args.commit)}
    if args.parent_root:
        sides["parent"] = (os.path.abspath(args.parent_root), args.parent_commit)
    reps = {side: [] for side in sides}
    for _ in range(args.repeats):  # parent, this, parent, this, ...
        for side in sorted(sides):
            reps[side].append(repeat(sides[side][0], "product", args.calls))
            print(side, reps[side][-1]["run_wall_median_ms"], reps[side][-1]["sv_traj_kernel_ms"], flush=True)
    res["product_model"] = {side: summary(sides[side][1], reps[side]) for side in sides}
    if "parent" in sides:
        p, t = res["product_model"]["parent"], res["product_model"]["this"]
        res["product_model"]["slower_by_ms"] = t["median_ms"] - p["median_ms"]
        res["product_model"]["within_parent_spread"] = bool(t["median_ms"] - p["median_ms"] <= p["spread_ms"])
    res["correlated_models"] = {}
    for variant in ("depolarize", "decay"):
        r = []
        for _ in range(args.repeats):
            r.append(repeat(ROOT, variant, args.calls))
            print(variant, r[-1]["run_wall_median_ms"], r[-1]["sv_traj_kernel_ms"], flush=True)
        res["correlated_models"][variant] = summary(args.commit, r)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(res, f, indent=1)
    print(json.dumps({k: v for k, v in res["product_model"].items() if not isinstance(v, dict)}))


if __name__ == "__main__":
    main()
