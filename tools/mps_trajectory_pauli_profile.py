"""The noisy Pauli readout on the MPS engine -> profiles/mps_trajectory_pauli.json.

Workload: 50 qubits, brickwork(50, 4, 50) (tests/sampling_ref.py) under create_noisemodel(50e-3, 70e-3)
-- the circuit and model of profiles/mps_trajectory.json -- and the 297 terms of
heisenberg_hamiltonian(50, 1, 0.8, 0.6, hx=0.3, hy=0.2, hz=0.5), 2048 shots.

The driver opens no GPU itself: every step is a child process of this script under its own ``timeout``,
and the first step that fails (or runs out of time) ends the run, nothing further being started.
Steps, every wall time ending in a device synchronise (each call returns host data):
1. ``device``: SamplingSimulator(method="matrix_product_state", mps_trajectories=True,
   mps_pauli_readout=True).pauli_counts of all terms (one aqc_mps_traj_pauli_counts call: the host's
   trajectory_program and readout_effects, 2048 trajectories, each read out for every term), the wall time
   of ``--reps`` calls after a warm-up; then one call with the HIP-event timers on, split into evolve
   (two-site kernels and k_mps_kraus1), environments ("traj_pauli_env"), chains
   ("mps_traj_pauli_chain") and draw ("mps_traj_pauli_draw");
2. ``readout_16`` .. ``readout_128``: the same call with aqc_mps_traj_set_readout_batch forcing R states
   per readout sweep, the wall time and the three readout families' event times;
3. ``circuits``: the only route of a build without the readout -- ``pauli_terms=None`` on the same
   simulator, one rotated noisy MPS trajectory run of 2048 shots per term -- timed on ``--baseline-terms``
   terms and SCALED to 297 (labelled so).

Usage: python tools/mps_trajectory_pauli_profile.py [--reps 3] [--shots 2048] [--out ...]
"""
import argparse
import json
import os
import subprocess
import sys
import tempfile
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

N, DEPTH = 50, 4
EVOLVE = ("mps_theta", "mps_svd", "mps_split", "mps_kraus1")
READOUT = ("traj_pauli_env", "mps_traj_pauli_chain", "mps_traj_pauli_draw")
R_VALUES = (16, 32, 64, 128)
STEP_SECONDS = {"device": 300, "circuits": 240}


def stats(ts):
    import numpy as np

    ts = np.asarray(ts) * 1e3
    q1, med, q3 = np.percentile(ts, [25, 50, 75])
    return {"median_ms": float(med), "min_ms": float(ts.min()), "q1_ms": float(q1), "q3_ms": float(q3),
            "max_ms": float(ts.max()), "reps": int(len(ts))}


def clock(fn):
    t0 = time.perf_counter()
    out = fn()
    return time.perf_counter() - t0, out


def workload(n):
    import sampling_ref as ref
    from adaptaqc_amd.utils.circuit_operations import create_noisemodel
    from adaptaqc_amd.utils.hamiltonians import heisenberg_hamiltonian
    from conftest import to_circuit

    nm = create_noisemodel(50e-3, 70e-3, log_fidelities=False)
    qc = to_circuit(n, ref.brickwork(n, DEPTH, n))
    labels = list(heisenberg_hamiltonian(n, 1.0, 0.8, 0.6, hx=0.3, hy=0.2, hz=0.5))
    return qc, nm, labels


def simulator():
    from adaptaqc_amd.backends.qiskit_sampling_backend import SamplingSimulator

    return SamplingSimulator(method="matrix_product_state", seed=1, mps_trajectories=True, mps_pauli_readout=True)


def events(call, families):
    from adaptaqc_amd import _lib

    _lib.timing_enable(True)
    _lib.timing_reset()
    call()
    q = {name: _lib.timing_query(name) for name in families}
    _lib.timing_enable(False)
    return q


def step_device(args, forced=0):
    """The device route; ``forced``: states per readout sweep (0: the default)."""
    from adaptaqc_amd import _lib
    from adaptaqc_amd.device import mps_trajectory_plan
    from adaptaqc_amd.mps_operations import chi_cap_for
    from adaptaqc_amd.noise import trajectory_program

    n = args.n
    qc, nm, labels = workload(n)
    sim = simulator()
    _lib.check(_lib.lib().aqc_mps_traj_set_readout_batch(forced))

    def call(shots=args.shots):
        return sim.pauli_counts(qc, labels, shots=shots, seed_simulator=5, noise_model=nm)

    call(min(args.shots, 64))  # warm-up of every shape
    wall = [clock(call)[0] for _ in range(args.reps)]
    q = events(call, EVOLVE + READOUT)
    res = {"wall": stats(wall), "readout_states_per_sweep_forced": forced,
           "readout_sweeps": int(q["mps_traj_pauli_draw"]["launches"]),
           "evolve_event_ms": sum(q[f]["ms"] for f in EVOLVE), "environments_event_ms": q["traj_pauli_env"]["ms"],
           "chains_event_ms": q["mps_traj_pauli_chain"]["ms"], "draw_event_ms": q["mps_traj_pauli_draw"]["ms"]}
    if not forced:
        rows, n_events, _ = trajectory_program(qc, nm)
        res.update({"n": n, "depth": DEPTH, "t1_ns": 50e3, "t2_ns": 70e3, "terms": len(labels), "shots": args.shots,
                    "chi_cap": chi_cap_for(n, None), "program_rows": int(len(rows)), "kraus_events": int(n_events),
                    "plan_without_measurement_sweep": mps_trajectory_plan(n, rows, measure=False)})
    return res


def step_circuits(args):
    """``pauli_terms=None``: one rotated circuit and one noisy MPS trajectory run per term."""
    from adaptaqc_amd.backends.qiskit_sampling_backend import QiskitSamplingBackend
    from adaptaqc_amd.utils.circuit_operations import expectation_values_of_pauli_terms

    qc, nm, labels = workload(args.n)
    be = QiskitSamplingBackend(simulator())
    kwargs = {"shots": args.shots, "seed_simulator": 5, "noise_model": nm}
    timed = [labels[0], labels[len(labels) // 2], labels[-1]][: args.baseline_terms]
    expectation_values_of_pauli_terms(qc, timed[:1], be, execute_kwargs=dict(kwargs, shots=64))  # warm-up
    wall = clock(lambda: expectation_values_of_pauli_terms(qc, timed, be, execute_kwargs=kwargs))[0]
    return {"terms_timed": len(timed), "wall_s": wall, "ms_per_term": 1e3 * wall / len(timed),
            "all_terms_ms_scaled": 1e3 * wall / len(timed) * len(labels), "scaled_to_terms": len(labels)}


def run_step(name, args, tmp):
    """One child process under its own time limit; its result, or None when it failed."""
    out = os.path.join(tmp, name + ".json")
    limit = STEP_SECONDS.get(name, 180)
    cmd = ["timeout", "-k", "10", str(limit), sys.executable, os.path.abspath(__file__), "--step", name, "--step-out", out,
           "--reps", str(args.reps), "--n", str(args.n), "--shots", str(args.shots), "--baseline-terms", str(args.baseline_terms)]
    rc = subprocess.call(cmd)
    if rc != 0 or not os.path.exists(out):
        print(f"step {name} failed with exit status {rc}: stopping", flush=True)
        return None
    with open(out) as f:
        return json.load(f)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--n", type=int, default=N)
    ap.add_argument("--shots", type=int, default=2048)
    ap.add_argument("--baseline-terms", type=int, default=3)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "mps_trajectory_pauli.json"))
    ap.add_argument("--step", default=None, help="(internal) run one step in this process")
    ap.add_argument("--step-out", default=None)
    args = ap.parse_args()

    if args.step:
        if args.step == "device":
            res = step_device(args)
        elif args.step.startswith("readout_"):
            res = step_device(args, int(args.step.split("_")[1]))
        else:
            res = step_circuits(args)
        print(json.dumps({args.step: res}), flush=True)
        with open(args.step_out, "w") as f:
            json.dump(res, f)
        return 0

    res = {}
    with tempfile.TemporaryDirectory() as tmp:
        for name in ("device",) + tuple(f"readout_{r}" for r in R_VALUES) + ("circuits",):
            got = run_step(name, args, tmp)
            if got is None:
                return 1
            res[name] = got
    res["readout_batch_wall_median_ms"] = {str(r): res[f"readout_{r}"]["wall"]["median_ms"] for r in R_VALUES}
    res["speedup_device_over_circuits_scaled"] = res["circuits"]["all_terms_ms_scaled"] / res["device"]["wall"]["median_ms"]
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(res, f, indent=1)
    print(json.dumps(res), flush=True)
    return 0


if __name__ == "__main__":
    sys.exit(main())
