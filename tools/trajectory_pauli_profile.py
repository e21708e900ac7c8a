"""The Pauli readout of noisy trajectories -> profiles/trajectory_pauli.json.

Input: the workload of tools/trajectory_profile.py at 13 qubits -- brickwork(13, 8, 13)
(tests/sampling_ref.py) under create_noisemodel(50e-3, 70e-3) -- and the 36 terms of
heisenberg_hamiltonian(13, 1, 1, 1), 8192 shots.

(a) The energy through expectation_value_of_pauli_operator with QiskitSamplingBackend(pauli_terms="device")
    (one aqc_sv_traj_pauli_counts launch: 8192 trajectories, each read out for every term) and with
    pauli_terms=None (one rotated circuit, i.e. one trajectory run, per term), on this tree.  A repeat is
    one fresh process: a warm-up of each route, then ``--calls`` timed calls of the device route and
    ``--circuit-calls`` of the per-term route; recorded: every repeat, the median over the repeats and
    their spread (max - min), and the HIP-event time of the sv_traj_pauli_counts kernel beside that of
    sv_traj for the same program (what the readout adds to the trajectories).
(b) The existing endings must not pay for the new one: aqc_sv_traj_sample (8192 shots) and
    aqc_sv_traj_pair_tomo (all 78 pairs, 910 shots a setting) on a checkout of the parent commit
    (--parent-root, with its own built library) and on this tree, in fresh processes that alternate.
    The change passes where its median lies within the parent's own spread above the parent's median.

Usage: python tools/trajectory_pauli_profile.py [--parent-root DIR] [--repeats 5] [--calls 9]
       [--circuit-calls 3] [--out profiles/trajectory_pauli.json]
"""
import argparse
import json
import os
import subprocess
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
N, DEPTH, SHOTS, TOMO_SHOTS = 13, 8, 8192, 910


def _setup(root):
    sys.path.insert(0, root)
    sys.path.insert(0, os.path.join(root, "tests"))
    import sampling_ref as ref
    from adaptaqc_amd.utils import circuit_operations as co
    from conftest import to_circuit

    return to_circuit(N, ref.brickwork(N, DEPTH, N)), co.create_noisemodel(50e-3, 70e-3, log_fidelities=False)


def _timed(call, calls):
    wall = []
    for _ in range(calls):
        t0 = time.perf_counter()
        call()
        wall.append((time.perf_counter() - t0) * 1e3)
    return wall


def _kernel_ms(_lib, name, call):
    _lib.timing_enable(True)
    _lib.timing_reset()
    for _ in range(3):
        call()
    k = _lib.timing_query(name)
    _lib.timing_enable(False)
    return k["ms"] / max(k["launches"], 1)


def worker_routes(root, calls, circuit_calls):
    """One repeat of (a), in this process: prints one JSON line."""
    qc, nm = _setup(root)
    from adaptaqc_amd import _lib
    from adaptaqc_amd.backends.qiskit_sampling_backend import QiskitSamplingBackend, SamplingSimulator
    from adaptaqc_amd.utils.circuit_operations import expectation_value_of_pauli_operator
    from adaptaqc_amd.utils.hamiltonians import heisenberg_hamiltonian

    ham = heisenberg_hamiltonian(N, 1.0, 1.0, 1.0)
    kwargs = {"shots": SHOTS, "seed_simulator": 5, "noise_model": nm}
    sim = SamplingSimulator(method="statevector", seed=1)
    device = QiskitSamplingBackend(sim, pauli_terms="device")
    circuits = QiskitSamplingBackend(sim)

    def run(backend):
        return expectation_value_of_pauli_operator(qc, ham, backend, execute_kwargs=kwargs)

    e_device, e_circuits = run(device), run(circuits)  # warm-up
    wall_device = _timed(lambda: run(device), calls)
    wall_circuits = _timed(lambda: run(circuits), circuit_calls)
    print(json.dumps({"terms": len(ham), "energy_device": e_device, "energy_circuits": e_circuits,
                      "device_wall_ms": wall_device, "device_wall_median_ms": float(np.median(wall_device)),
                      "circuits_wall_ms": wall_circuits, "circuits_wall_median_ms": float(np.median(wall_circuits)),
                      "sv_traj_pauli_counts_kernel_ms": _kernel_ms(_lib, "sv_traj_pauli_counts", lambda: run(device)),
                      "sv_traj_kernel_ms": _kernel_ms(
                          _lib, "sv_traj", lambda: sim.run(qc, shots=SHOTS, seed_simulator=5, noise_model=nm))}),
          flush=True)


def worker_existing(root, calls):
    """One repeat of (b), in this process (nothing the parent commit lacks): prints one JSON line."""
    qc, nm = _setup(root)
    from adaptaqc_amd import _lib, noise
    from adaptaqc_amd.device import trajectory_pair_tomography, trajectory_sample

    rows, n_events, _ = noise.trajectory_program(qc, nm)
    effects = noise.readout_effects(N, nm)
    pairs = [(a, b) for a in range(N) for b in range(a + 1, N)]

    def sample():
        return trajectory_sample(N, rows, n_events, SHOTS, 5)

    def tomo():
        return trajectory_pair_tomography(N, rows, n_events, pairs, effects, TOMO_SHOTS, 5)

    first, table = sample(), tomo()  # warm-up
    wall_sample = _timed(sample, calls)
    wall_tomo = _timed(tomo, calls)
    print(json.dumps({"program_rows": int(len(rows)), "events": int(n_events), "pairs": len(pairs),
                      "sample_wall_ms": wall_sample, "sample_wall_median_ms": float(np.median(wall_sample)),
                      "pair_tomo_wall_ms": wall_tomo, "pair_tomo_wall_median_ms": float(np.median(wall_tomo)),
                      "sv_traj_kernel_ms": _kernel_ms(_lib, "sv_traj", sample),
                      "sv_traj_pair_tomo_kernel_ms": _kernel_ms(_lib, "sv_traj_pair_tomo", tomo),
                      "sample_checksum": int(first.sum() % (1 << 32)), "tomo_checksum": int(table.sum())}), flush=True)


def repeat(root, worker, calls, circuit_calls):
    out = subprocess.run([sys.executable, os.path.abspath(__file__), "--worker", worker, "--root", root,
                          "--calls", str(calls), "--circuit-calls", str(circuit_calls)],
                         capture_output=True, text=True, timeout=600)
    if out.returncode != 0:
        raise RuntimeError(f"{worker} in {root} ended with status {out.returncode}:\n{out.stderr[-2000:]}")
    return json.loads(out.stdout.strip().splitlines()[-1])


def spread(reps, key):
    v = [r[key] for r in reps]
    return {"median_ms": float(np.median(v)), "spread_ms": float(max(v) - min(v))}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--parent-root", default=None, help="a built checkout of the parent commit")
    ap.add_argument("--parent-commit", default="parent")
    ap.add_argument("--commit", default="this change")
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--calls", type=int, default=9)
    ap.add_argument("--circuit-calls", type=int, default=3)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "trajectory_pauli.json"))
    ap.add_argument("--worker", default=None)
    ap.add_argument("--root", default=ROOT)
    args = ap.parse_args()
    if args.worker == "routes":
        worker_routes(os.path.abspath(args.root), args.calls, args.circuit_calls)
        return
    if args.worker == "existing":
        worker_existing(os.path.abspath(args.root), args.calls)
        return

    res = {"n": N, "depth": DEPTH, "shots": SHOTS, "pair_tomography_shots_per_setting": TOMO_SHOTS,
           "calls_per_repeat": args.calls, "circuit_route_calls_per_repeat": args.circuit_calls,
           "what": "wall times; a repeat is one fresh process"}
    # (b) first, alternating: parent, this, parent, this, ...
    sides = {"this": (ROOT, args.commit)}
    if args.parent_root:
        sides["parent"] = (os.path.abspath(args.parent_root), args.parent_commit)
    reps = {side: [] for side in sides}
    for _ in range(args.repeats):
        for side in sorted(sides):
            reps[side].append(repeat(sides[side][0], "existing", args.calls, args.circuit_calls))
            print(side, reps[side][-1]["sample_wall_median_ms"], reps[side][-1]["pair_tomo_wall_median_ms"], flush=True)
    existing = {}
    for entry, key, kernel in (("aqc_sv_traj_sample", "sample_wall_median_ms", "sv_traj_kernel_ms"),
                               ("aqc_sv_traj_pair_tomo", "pair_tomo_wall_median_ms", "sv_traj_pair_tomo_kernel_ms")):
        existing[entry] = {side: dict(spread(reps[side], key), commit=sides[side][1],
                                      kernel=spread(reps[side], kernel)) for side in sides}
        if "parent" in sides:
            p, t = existing[entry]["parent"], existing[entry]["this"]
            existing[entry]["slower_by_ms"] = t["median_ms"] - p["median_ms"]
            existing[entry]["within_parent_spread"] = bool(t["median_ms"] - p["median_ms"] <= p["spread_ms"])
    existing["repeats"] = reps
    res["existing_endings"] = existing
    # (a)
    routes = []
    for _ in range(args.repeats):
        routes.append(repeat(ROOT, "routes", args.calls, args.circuit_calls))
        print("routes", routes[-1]["device_wall_median_ms"], routes[-1]["circuits_wall_median_ms"], flush=True)
    dev, circ = spread(routes, "device_wall_median_ms"), spread(routes, "circuits_wall_median_ms")
    res["routes"] = {"terms": routes[0]["terms"], "device": dev, "circuits": circ,
                     "ratio_of_medians": circ["median_ms"] / dev["median_ms"],
                     "sv_traj_pauli_counts_kernel": spread(routes, "sv_traj_pauli_counts_kernel_ms"),
                     "sv_traj_kernel": spread(routes, "sv_traj_kernel_ms"), "repeats": routes}
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(res, f, indent=1)
    print(json.dumps({"device_ms": dev, "circuits_ms": circ, "ratio": res["routes"]["ratio_of_medians"],
                      "existing": {k: {s: v[s] for s in ("slower_by_ms", "within_parent_spread") if s in v}
                                   for k, v in existing.items() if k != "repeats"}}))


if __name__ == "__main__":
    main()
