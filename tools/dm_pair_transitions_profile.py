"""The pair-transition reader and the general_gradient route it opens -> profiles/dm_pair_transitions.json.

Input: the circuit of profiles/dm_gradient.json -- brickwork(n, 8, n) (tests/sampling_ref.py) under
create_noisemodel(50e-3, 70e-3) -- for n = 8, 10, 12 as the target of an AdaptCompiler on DensityMatrixBackend with
method="general_gradient" and the full coupling map (n (n - 1) / 2 pairs), once with a product starting circuit
and once with an entangling one (the product circuit followed by a ladder of cx).  On the evolved rho in front of
the first layer and the cost observable M pulled back through the entangling right-hand side:
(a) DeviceDM.pair_transitions(M, rho) over all pairs: wall time and the kernel's HIP-event time, per pair;
(b) DeviceDM.transition(M, rho, q) on the same two matrices (it reads the same 2 x 16 x 4^n bytes as one pair of
    (a)): the ratio (a) per pair / (b), and both as a fraction of the measured HBM copy rate (below 12 qubits the
    two matrices fit the Infinity Cache and the fraction is not an HBM figure; at 12 they are twice its size and
    every pair re-reads them);
(c) the whole general_gradients call on the product start: the two-matrix route (pair_transitions="always")
    against the effects route, for the global cost, and the two-matrix route for the local cost;
(d) the whole call on the entangling start, both costs, against the generic route for two pairs -- one
    DeviceDM.run of the whole program per shifted candidate, 24 a pair -- scaled to all pairs and labelled as
    scaled;
(e) the backward pass that makes M (once a compile).
Wall times are the minimum of --reps repetitions, with the spread; kernel times are the minimum over --reps
passes of their own.

Usage: python tools/dm_pair_transitions_profile.py [--reps 5] [--sizes 8 10 12] [--out profiles/dm_pair_transitions.json]
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


def kernel_ms(name, fn, reps):
    """The HIP-event time of one launch of ``name`` inside ``fn``: the minimum over ``reps`` timed passes."""
    from adaptaqc_amd import _lib

    fn()  # warm-up
    best = None
    for _ in range(reps):
        _lib.timing_enable(True)
        _lib.timing_reset()
        fn()
        k = _lib.timing_query(name)
        _lib.timing_enable(False)
        ms = k["ms"] / max(1, k["launches"])
        best = ms if best is None else min(best, ms)
    return best


def starting_circuit(n, seed, entangling):
    from adaptaqc_amd.circuit import QuantumCircuit

    rng = np.random.default_rng(seed)
    qc = QuantumCircuit(n)
    for q in range(n):
        qc.ry(float(rng.uniform(0.2, 1.2)), q)
        qc.rz(float(rng.uniform(0.2, 1.2)), q)
    if entangling:
        for q in range(n - 1):
            qc.cx(q, q + 1)
    return qc


def build(n, nm, entangling, **backend_kw):
    import sampling_ref as ref
    from adaptaqc_amd.backends import DensityMatrixBackend
    from adaptaqc_amd.compilers import AdaptCompiler, AdaptConfig
    from conftest import to_circuit

    return AdaptCompiler(to_circuit(n, ref.brickwork(n, DEPTH, n)), backend=DensityMatrixBackend(**backend_kw),
                         adapt_config=AdaptConfig(method="general_gradient"), execute_kwargs={"noise_model": nm},
                         starting_circuit=starting_circuit(n, 900 + n, entangling))


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


def release(backend):
    for cache in (backend._evolved, backend._evolved_left):
        if cache._last is not None:
            cache._last[2].close()
            cache._last = None
    for _, dev in (backend._observables or {}).values():
        dev.close()
    backend._observables = {}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--sizes", type=int, nargs="+", default=[8, 10, 12])
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "dm_pair_transitions.json"))
    args = ap.parse_args()

    from adaptaqc_amd.device import dm_pair_transitions_split
    from adaptaqc_amd.utils.circuit_operations import create_noisemodel

    nm = create_noisemodel(50e-3, 70e-3, log_fidelities=False)
    res = {"t1_ns": 50e3, "t2_ns": 70e3, "depth": DEPTH, "hbm_copy_tb_per_s": HBM_COPY_TBS, "sizes": []}
    for n in args.sizes:
        ent = build(n, nm, True, pair_transitions=True)
        pairs = [(int(a), int(b)) for a, b in ent.coupling_map]
        be = ent.backend
        t0 = time.perf_counter()
        be.pair_transition_matrices(ent, pairs[:1], "global")  # evolves rho and pulls M back
        first_ms = (time.perf_counter() - t0) * 1e3
        rho = be._evolved_left._last[2]
        obs = be._observables["global"][1]
        bytes_pair = 2 * 16 * 4 ** n
        r = {"n": n, "matrix_bytes": 16 * 4 ** n, "pairs": len(pairs), "bytes_per_pair": bytes_pair,
             "workgroups_per_pair": dm_pair_transitions_split(n, len(pairs)),
             "first_call_with_evolution_and_backward_pass_ms": first_ms}
        r["a_pair_transitions_wall"] = timed(lambda: obs.pair_transitions(rho, pairs), args.reps)
        r["a_kernel_ms"] = kernel_ms("dm_pair_transitions", lambda: obs.pair_transitions(rho, pairs), args.reps)
        r["a_kernel_ms_per_pair"] = r["a_kernel_ms"] / len(pairs)
        r["a_one_pair_kernel_ms"] = kernel_ms("dm_pair_transitions", lambda: obs.pair_transitions(rho, pairs[:1]), args.reps)
        r["b_transition_wall"] = timed(lambda: obs.transition(rho, n // 2), args.reps)
        r["b_kernel_ms"] = kernel_ms("dm_transition", lambda: obs.transition(rho, n // 2), args.reps)
        r["a_per_pair_over_b_kernel"] = r["a_kernel_ms_per_pair"] / r["b_kernel_ms"]
        r["a_one_pair_over_b_kernel"] = r["a_one_pair_kernel_ms"] / r["b_kernel_ms"]
        r["a_tb_per_s"] = bytes_pair / (r["a_kernel_ms_per_pair"] * 1e-3) / 1e12
        r["a_fraction_of_copy_rate"] = r["a_tb_per_s"] / HBM_COPY_TBS
        r["a_one_pair_fraction_of_copy_rate"] = bytes_pair / (r["a_one_pair_kernel_ms"] * 1e-3) / 1e12 / HBM_COPY_TBS
        r["a_fp64_tflops"] = 2048.0 * 4 ** (n - 2) / (r["a_kernel_ms_per_pair"] * 1e-3) / 1e12
        r["b_fraction_of_copy_rate"] = bytes_pair / (r["b_kernel_ms"] * 1e-3) / 1e12 / HBM_COPY_TBS
        r["working_set"] = ("both matrices fit the 256 MiB Infinity Cache: the fractions are not HBM figures"
                            if bytes_pair <= 2 ** 28 else "the two matrices are twice the 256 MiB Infinity Cache")

        def backward():
            be._observables = {}
            be.pair_transition_matrices(ent, pairs[:1], "global")

        r["e_backward_pass_and_one_pair_wall"] = timed(backward, max(2, args.reps // 2))
        # (d) the entangling start
        r["d_gradient_call_entangling_global_wall"] = timed(lambda: be.general_gradients(ent), args.reps)
        be.gradient_cost = "local"
        r["d_gradient_call_entangling_local_wall"] = timed(lambda: be.general_gradients(ent), args.reps)
        be.gradient_cost = "global"
        wall, evolutions = generic_route(ent, nm, pairs[:GENERIC_PAIRS], max(2, args.reps // 2))
        r["d_generic_two_pairs_wall"] = wall
        r["d_generic_evolutions_measured"] = evolutions
        r["d_generic_all_pairs_scaled_ms"] = wall["min_ms"] * len(pairs) / GENERIC_PAIRS
        r["d_is_scaled_from_pairs"] = GENERIC_PAIRS
        r["speedup_scaled_generic_over_gradient_call"] = (r["d_generic_all_pairs_scaled_ms"]
                                                          / r["d_gradient_call_entangling_global_wall"]["min_ms"])
        release(be)
        # (c) the product start
        effects, always = build(n, nm, False), build(n, nm, False, pair_transitions="always")
        r["c_gradient_call_product_effects_wall"] = timed(lambda: effects.backend.general_gradients(effects), args.reps)
        r["c_gradient_call_product_two_matrix_wall"] = timed(lambda: always.backend.general_gradients(always), args.reps)
        always.backend.gradient_cost = "local"
        r["c_gradient_call_product_two_matrix_local_wall"] = timed(lambda: always.backend.general_gradients(always), args.reps)
        r["c_two_matrix_over_effects"] = (r["c_gradient_call_product_two_matrix_wall"]["min_ms"]
                                          / r["c_gradient_call_product_effects_wall"]["min_ms"])
        local_max = float(np.max(always.backend.general_gradients(always)))  # (local: no second route to compare)
        always.backend.gradient_cost = "global"
        r["c_routes_max_gap"] = float(np.max(np.abs(np.array(always.backend.general_gradients(always))
                                                    - np.array(effects.backend.general_gradients(effects)))))
        r["c_local_gradient_max"] = local_max
        release(effects.backend)
        release(always.backend)
        res["sizes"].append(r)
        print(json.dumps(r), flush=True)

    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(res, f, indent=1)


if __name__ == "__main__":
    main()
