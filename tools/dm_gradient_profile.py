"""Noise-aware general_gradient pair selection on the density-matrix engine -> profiles/dm_gradient.json.

Input: the circuit of profiles/density_matrix.json -- brickwork(n, 8, n) (tests/sampling_ref.py) under
create_noisemodel(50e-3, 70e-3) -- for n = 8, 10, 12 as the target of an AdaptCompiler on
DensityMatrixBackend with method="general_gradient" and the full coupling map (n (n - 1) / 2 pairs).  On the
evolved rho in front of the first layer:
(a) DeviceDM.pair_envs over all pairs with the model's effects (the error on measure: all diagonal);
(b) the same with the effects behind a random product starting circuit (every effect with an off-diagonal);
(c) DeviceDM.pair_rdms on the same pairs, which reads the bytes of (a);
(d) the whole gradient call (DensityMatrixBackend.general_gradients, rho cached), for (a)'s and (b)'s compiler;
(e) the generic route for two pairs -- one DeviceDM.run of the whole program per shifted candidate, 24 a
    pair -- scaled to all pairs and labelled as scaled.
Wall times are the minimum of --reps repetitions, with the spread; the kernels' HIP-event times come from a
pass of their own.  (a) is judged against (c); (b) against 4^(n-2) x 16 x 16 bytes a pair at the measured
HBM copy rate (up to 12 qubits rho fits, or nearly fits, the Infinity Cache: the share is then not an HBM
figure).

Usage: python tools/dm_gradient_profile.py [--reps 5] [--out profiles/dm_gradient.json]
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
GENERIC_PAIRS = 2


def spread(ts):
    ts = np.asarray(ts) * 1e3
    return {"min_ms": float(ts.min()), "median_ms": float(np.median(ts)), "max_ms": float(ts.max()), "reps": int(len(ts))}


def timed(fn, reps):
    fn()  # warm-up
    ts = []
    for _ in range(reps):
        t0 = time.perf_counter()
        fn()
        ts.append(time.perf_counter() - t0)
    return spread(ts)


def product_circuit(n, seed):
    from adaptaqc_amd.circuit import QuantumCircuit

    rng = np.random.default_rng(seed)
    qc = QuantumCircuit(n)
    for q in range(n):
        qc.ry(float(rng.uniform(0.2, 1.2)), q)
        qc.rz(float(rng.uniform(0.2, 1.2)), q)
    return qc


def build(n, nm, start):
    import sampling_ref as ref
    from adaptaqc_amd.backends import DensityMatrixBackend
    from adaptaqc_amd.compilers import AdaptCompiler, AdaptConfig
    from conftest import to_circuit

    return AdaptCompiler(to_circuit(n, ref.brickwork(n, DEPTH, n)), backend=DensityMatrixBackend(),
                         adapt_config=AdaptConfig(method="general_gradient"), execute_kwargs={"noise_model": nm},
                         starting_circuit=product_circuit(n, 900 + n) if start else None)


def kernel_ms(name, fn):
    from adaptaqc_amd import _lib

    _lib.timing_enable(True)
    _lib.timing_reset()
    fn()
    k = _lib.timing_query(name)
    _lib.timing_enable(False)
    return k["ms"] / max(1, k["launches"])


def generic_route(comp, nm, pairs, reps):
    """One DeviceDM.run of the whole program per shifted candidate of ``pairs``: (wall spread, evolutions)."""
    from adaptaqc_amd.device import DeviceDM
    from adaptaqc_amd.noise import trajectory_program
    from adaptaqc_amd.utils import circuit_operations as co
    from adaptaqc_amd.utils.gradients import shifted_layers

    n = comp.full_circuit.num_qubits
    end = comp.variational_circuit_range()[1]
    cands = shifted_layers(comp.layer_2q_gate, True, np.pi / 2) + shifted_layers(comp.layer_2q_gate, True, -np.pi / 2)
    dev = DeviceDM(n)

    def run():
        for c, t in pairs:
            for cand in cands:
                qc = comp.full_circuit.copy()
                co.add_to_circuit(qc, cand, end, qubit_subset=[c, t])
                for q in range(n):
                    qc.measure(q, q)
                rows, _, _ = trajectory_program(qc, nm)
                dev.reset()
                dev.run(rows)
                dev.prob0()

    out = timed(run, reps)
    dev.close()
    return out, len(pairs) * len(cands)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "dm_gradient.json"))
    args = ap.parse_args()

    from adaptaqc_amd.utils.circuit_operations import create_noisemodel

    nm = create_noisemodel(50e-3, 70e-3, log_fidelities=False)
    res = {"t1_ns": 50e3, "t2_ns": 70e3, "depth": DEPTH, "hbm_copy_tb_per_s": HBM_COPY_TBS, "sizes": []}
    for n in SIZES:
        plain, started = build(n, nm, False), build(n, nm, True)
        pairs = [(int(a), int(b)) for a, b in plain.coupling_map]
        _, _, eff_a = plain.backend.pair_environments(plain, pairs[:1])
        _, _, eff_b = started.backend.pair_environments(started, pairs[:1])
        dev = plain.backend._evolved_left._last[2]  # rho in front of the first layer
        r = {"n": n, "rho_bytes": 16 * 4 ** n, "pairs": len(pairs),
             "effects_a_with_off_diagonal": int(np.count_nonzero(np.any(eff_a[:, 2:] != 0, axis=1))),
             "effects_b_with_off_diagonal": int(np.count_nonzero(np.any(eff_b[:, 2:] != 0, axis=1)))}
        r["a_pair_envs_diagonal_wall"] = timed(lambda: dev.pair_envs(pairs, eff_a), args.reps)
        r["b_pair_envs_full_wall"] = timed(lambda: dev.pair_envs(pairs, eff_b), args.reps)
        r["c_pair_rdms_wall"] = timed(lambda: dev.pair_rdms(pairs), args.reps)
        r["a_kernel_ms"] = kernel_ms("dm_pair_envs", lambda: dev.pair_envs(pairs, eff_a))
        r["b_kernel_ms"] = kernel_ms("dm_pair_envs", lambda: dev.pair_envs(pairs, eff_b))
        r["c_kernel_ms"] = kernel_ms("dm_pair_rdms", lambda: dev.pair_rdms(pairs))
        r["a_over_c_wall"] = r["a_pair_envs_diagonal_wall"]["min_ms"] / r["c_pair_rdms_wall"]["min_ms"]
        r["a_over_c_kernel"] = r["a_kernel_ms"] / r["c_kernel_ms"]
        r["b_bytes"] = len(pairs) * 4 ** (n - 2) * 16 * 16
        r["b_traffic_bound_ms"] = r["b_bytes"] / (HBM_COPY_TBS * 1e12) * 1e3
        r["b_kernel_tb_per_s"] = r["b_bytes"] / (r["b_kernel_ms"] * 1e-3) / 1e12
        r["b_share_of_traffic_bound"] = r["b_traffic_bound_ms"] / r["b_kernel_ms"]
        r["working_set"] = ("rho fits the 256 MiB Infinity Cache: the share is not an HBM figure" if 16 * 4 ** n < 2 ** 28
                            else "rho is 256 MiB, the size of the Infinity Cache")
        r["d_gradient_call_wall"] = timed(lambda: plain.backend.general_gradients(plain), args.reps)
        r["d_gradient_call_started_wall"] = timed(lambda: started.backend.general_gradients(started), args.reps)
        wall, evolutions = generic_route(plain, nm, pairs[:GENERIC_PAIRS], max(2, args.reps // 2))
        r["e_generic_two_pairs_wall"] = wall
        r["e_generic_evolutions_measured"] = evolutions
        r["e_generic_all_pairs_scaled_ms"] = wall["min_ms"] * len(pairs) / GENERIC_PAIRS
        r["e_is_scaled_from_pairs"] = GENERIC_PAIRS
        r["speedup_scaled_generic_over_gradient_call"] = r["e_generic_all_pairs_scaled_ms"] / r["d_gradient_call_wall"]["min_ms"]
        res["sizes"].append(r)
        print(json.dumps(r), flush=True)
        for comp in (plain, started):
            comp.backend._evolved_left._last[2].close()

    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(res, f, indent=1)


if __name__ == "__main__":
    main()
