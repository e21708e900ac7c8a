"""Heisenberg-picture Rotoselect sweep on the density-matrix engine -> profiles/dm_sweep.json.

Input: the circuit of profiles/density_matrix.json -- brickwork(n, 8, n) (tests/sampling_ref.py) under
create_noisemodel(50e-3, 70e-3) -- for n = 8, 10, 12, its last layer placed in the compiler's variational
range.  One Rotoselect cycle (CostMinimiser._reduce_cost) over that layer's n rotation gates, from the same
circuit every time:
1. with DensityMatrixBackend(heisenberg_sweep=True): one backward pass with a checkpoint per gate, the
   prefix pushed forward once, one aqc_dm_transition per gate;
2. with the default backend and use_cached_rotations = False: the generic path, 7 evolutions of rho per gate.
The minimum of --reps repetitions each, with the spread.  Then, in a cycle of its own, the HIP-event times
of the "dm_transition" and "dm_segment" launches of the sweep: k_dm_transition reads 2 x 16 x 4^n bytes,
which gives its share of the measured HBM copy rate (up to 12 qubits both matrices fit the Infinity Cache,
so the share is then not an HBM figure).  The count-derived ratio is the generic path's evolutions over
the sweep's two (one backward, one forward).

Usage: python tools/dm_sweep_profile.py [--reps 5] [--out profiles/dm_sweep.json]
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

SIZES = (8, 10, 12)
DEPTH = 8
HBM_COPY_TBS = 6.29  # the measured HBM copy rate of an MI355X


def spread(ts):
    ts = np.asarray(ts) * 1e3
    return {"min_ms": float(ts.min()), "median_ms": float(np.median(ts)), "max_ms": float(ts.max()), "reps": int(len(ts))}


def build(n, backend, nm):
    """(compiler, the range of the last layer): the first 7 layers as the target, the 8th in the
    variational range with labelled rotations, as an ADAPT layer's."""
    import sampling_ref as ref
    from adaptaqc_amd.circuit import Operation
    from adaptaqc_amd.compilers import AdaptCompiler
    from adaptaqc_amd.utils import circuit_operations as co
    from conftest import to_circuit

    ops = ref.brickwork(n, DEPTH, n)
    per_layer = [n + len(range(layer % 2, n - 1, 2)) for layer in range(DEPTH)]
    head = sum(per_layer[:-1])
    comp = AdaptCompiler(to_circuit(n, ops[:head]), backend=backend, execute_kwargs={"noise_model": nm})
    pos = len(comp.full_circuit.data) - comp.rhs_gate_count
    for k, (name, qs, params) in enumerate(ops[head:]):
        gate = co.create_1q_gate(name, params[0]) if len(qs) == 1 else Operation(name, 2, [])
        co.add_gate(comp.full_circuit, gate, pos + k, list(qs))
    return comp, (pos, pos + len(ops) - head)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "dm_sweep.json"))
    args = ap.parse_args()

    from adaptaqc_amd import _lib
    from adaptaqc_amd.backends import DensityMatrixBackend
    from adaptaqc_amd.device import DeviceDM
    from adaptaqc_amd.utils.circuit_operations import create_noisemodel

    nm = create_noisemodel(50e-3, 70e-3, log_fidelities=False)
    res = {"t1_ns": 50e3, "t2_ns": 70e3, "depth": DEPTH, "hbm_copy_tb_per_s": HBM_COPY_TBS, "sizes": []}
    for n in SIZES:
        sweep, rng = build(n, DensityMatrixBackend(heisenberg_sweep=True), nm)
        generic, grng = build(n, DensityMatrixBackend(), nm)
        generic.use_cached_rotations = False
        assert rng == grng
        start = list(sweep.full_circuit.data)

        def cycle(comp):
            comp.full_circuit.data[:] = start
            count = comp.cost_evaluation_counter
            t0 = time.perf_counter()
            cost = comp.minimizer._reduce_cost(True, rng)
            return time.perf_counter() - t0, cost, comp.cost_evaluation_counter - count

        cycle(sweep), cycle(generic)  # warm-up of both paths
        ts, tg = [], []
        for _ in range(args.reps):  # alternating, so that both series see the same machine state
            t, cost_s, evals_s = cycle(sweep)
            ts.append(t)
            t, cost_g, evals_g = cycle(generic)
            tg.append(t)
        gates = evals_g // 7
        r = {"n": n, "rho_bytes": 16 * 4 ** n, "rotation_gates": int(gates), "generic_evolutions": int(evals_g),
             "sweep_counted_evaluations": int(evals_s), "cost_after_cycle_sweep": cost_s,
             "cost_after_cycle_generic": cost_g, "cost_difference": abs(cost_s - cost_g),
             "sweep_cycle_wall": spread(ts), "generic_cycle_wall": spread(tg)}
        r["measured_ratio"] = r["generic_cycle_wall"]["min_ms"] / r["sweep_cycle_wall"]["min_ms"]
        r["count_derived_ratio"] = evals_g / 2
        r["faster_by_more_than_the_spread"] = bool(r["sweep_cycle_wall"]["max_ms"] < r["generic_cycle_wall"]["min_ms"])

        _lib.timing_enable(True)
        _lib.timing_reset()
        cycle(sweep)
        kt, ks = _lib.timing_query("dm_transition"), _lib.timing_query("dm_segment")
        _lib.timing_enable(False)
        ms = kt["ms"] / max(1, kt["launches"])
        r["dm_transition_launches"] = int(kt["launches"])
        r["dm_transition_kernel_ms"] = ms
        r["dm_transition_bytes"] = 2 * 16 * 4 ** n
        r["dm_transition_tb_per_s"] = r["dm_transition_bytes"] / (ms * 1e-3) / 1e12
        r["dm_transition_share_of_hbm_copy_rate"] = r["dm_transition_tb_per_s"] / HBM_COPY_TBS
        r["working_set"] = "both matrices fit the 256 MiB Infinity Cache: the share is not an HBM figure"
        r["sweep_dm_segment_launches"] = int(ks["launches"])
        r["sweep_dm_segment_kernels_ms"] = ks["ms"]
        a, b = DeviceDM(n), DeviceDM(n)
        a.copy_from(b)
        copies = []
        for _ in range(args.reps):
            t0 = time.perf_counter()
            a.copy_from(b)
            copies.append(time.perf_counter() - t0)
        r["checkpoint_copy_wall"] = spread(copies)
        a.close(), b.close()
        res["sizes"].append(r)
        print(json.dumps(r), flush=True)

    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(res, f, indent=1)


if __name__ == "__main__":
    main()
