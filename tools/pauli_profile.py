"""Pauli-operator expectation measurements -> profiles/pauli.json.

Input: the bench's 50-qubit chi = 64 state (bench.near_product_mps) and the 297-term Heisenberg
operator heisenberg_hamiltonian(50, 1, 1, 1, 1, 1, 1).

1. wall time per aqc_mps_pauli_expect call on one state (DeviceMPS.pauli_expect);
2. wall time per aqc_mps_pauli_expect_batch call on 8 states;
3. the HIP-event time of the call's two parts: the environment chains ("pauli_env") and the term
   chains ("pauli_chain"), from aqc_timing_query;
4. the only route to the same numbers before these kernels: DeviceMPS.pair_rdms over the 49
   neighbour pairs with the terms traced on the host, timed in the same process on the same state,
   alternating with (1) call by call; the two routes' values are compared;
5. the statevector kernel at n = 20 with the same operator (117 terms): wall time, HIP-event time
   and achieved bytes/s (32 bytes per amplitude and term: psi[k] and psi[k ^ x]).

Every wall time ends in a device synchronise (the calls return host results).  The spread of each
series is recorded (quartiles over the repetitions) so that a difference can be read against it.

Usage: python tools/pauli_profile.py [--reps 15] [--out profiles/pauli.json]
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
import bench  # noqa: E402

PAULI = {
    "X": np.array([[0, 1], [1, 0]], dtype=complex),
    "Y": np.array([[0, -1j], [1j, 0]], dtype=complex),
    "Z": np.array([[1, 0], [0, -1]], dtype=complex),
}


def stats(ts):
    ts = np.asarray(ts) * 1e3
    q1, med, q3 = np.percentile(ts, [25, 50, 75])
    return {"median_ms": float(med), "min_ms": float(ts.min()), "q1_ms": float(q1), "q3_ms": float(q3),
            "max_ms": float(ts.max()), "reps": int(len(ts))}


def clock(fn):
    t0 = time.perf_counter()
    out = fn()
    return time.perf_counter() - t0, out


def rdm_route(state, n):
    """{label: value} of the Heisenberg terms from the neighbour-pair RDMs (row index 2 bit(i+1) +
    bit(i)); single-site terms from the pair's partial trace."""
    pairs = [(i, i + 1) for i in range(n - 1)]
    rdms = state.pair_rdms(pairs)
    eye = np.eye(2)
    out = {}

    def label(ops):
        chars = ["I"] * n
        for q, p in ops:
            chars[n - 1 - q] = p
        return "".join(chars)

    for i, rho in enumerate(rdms):
        for p, m in PAULI.items():
            out[label([(i, p), (i + 1, p)])] = np.trace(rho @ np.kron(m, m)).real
            out[label([(i, p)])] = np.trace(rho @ np.kron(eye, m)).real
            if i == n - 2:
                out[label([(i + 1, p)])] = np.trace(rho @ np.kron(m, eye)).real
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=15)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "pauli.json"))
    args = ap.parse_args()

    import sampling_ref as ref
    from adaptaqc_amd import _lib, paulis
    from adaptaqc_amd.circuit import device_ops
    from adaptaqc_amd.device import DeviceMPS, DeviceSV, pauli_expect_batch
    from adaptaqc_amd.utils.hamiltonians import heisenberg_hamiltonian
    from conftest import to_circuit

    reps = args.reps
    peak = float(getattr(bench, "FP64_PEAK_TFLOPS", 78.6))
    res = {"fp64_matrix_peak_tflops": peak}

    # ---- MPS: the bench's 50-qubit chi = 64 state ------------------------------------------------
    n, chi = bench.N_QUBITS, 64
    labels = list(heisenberg_hamiltonian(n, 1, 1, 1, 1, 1, 1))
    codes = paulis.terms_to_codes(labels, n)
    base = DeviceMPS(n, chi, 1e-16, chi)
    base.load_aer(bench.near_product_mps(n, chi, 1000))
    copies = [DeviceMPS(n, chi, 1e-16, chi) for _ in range(8)]
    for c in copies:
        c.copy_from(base)
    mps = {"n": n, "chi": chi, "terms": len(labels), "max_bond": int(base.dims().max())}

    # warm-up of every shape, and the two routes' values against each other
    new = base.pauli_expect(codes)
    old = rdm_route(base, n)
    mps["max_abs_difference_between_routes"] = float(np.max(np.abs(new - np.array([old[l] for l in labels]))))
    batch = pauli_expect_batch(copies, codes)
    mps["batch_rows_equal_single_call"] = bool(all(np.array_equal(r, new) for r in batch))

    t_new, t_old, t_batch = [], [], []
    for _ in range(reps):  # alternating: both routes see the same machine state
        t_new.append(clock(lambda: base.pauli_expect(codes))[0])
        t_old.append(clock(lambda: rdm_route(base, n))[0])
        t_batch.append(clock(lambda: pauli_expect_batch(copies, codes))[0])
    mps["pauli_expect_wall"] = stats(t_new)
    mps["pair_rdms_route_wall"] = stats(t_old)
    mps["pauli_expect_batch8_wall"] = stats(t_batch)
    mps["new_over_rdm_route_median"] = mps["pauli_expect_wall"]["median_ms"] / mps["pair_rdms_route_wall"]["median_ms"]

    _lib.timing_enable(True)
    _lib.timing_reset()
    for _ in range(reps):
        base.pauli_expect(codes)
    env, ker = _lib.timing_query("pauli_env"), _lib.timing_query("pauli_chain")
    _lib.timing_reset()
    for _ in range(reps):
        pauli_expect_batch(copies, codes)
    env8, ker8 = _lib.timing_query("pauli_env"), _lib.timing_query("pauli_chain")
    _lib.timing_reset()
    for _ in range(reps):
        base.pair_rdms([(i, i + 1) for i in range(n - 1)])
    renv, rchain = _lib.timing_query("rdm_env"), _lib.timing_query("rdm_chain")
    _lib.timing_enable(False)

    def per(q):
        return q["ms"] / max(q["launches"], 1)

    mps["env_ms"] = per(env)
    mps["chain_ms"] = per(ker)
    mps["env_share"] = per(env) / (per(env) + per(ker))
    mps["chain_tflops_nominal_cap"] = ker["flops"] / max(ker["launches"], 1) / (per(ker) * 1e-3) / 1e12
    mps["batch8_env_ms"] = per(env8)
    mps["batch8_chain_ms"] = per(ker8)
    mps["rdm_route_env_ms"] = per(renv)
    mps["rdm_route_chain_ms"] = per(rchain)
    res["mps"] = mps

    # ---- statevector: 20-qubit brickwork ---------------------------------------------------------
    n = 20
    labels = list(heisenberg_hamiltonian(n, 1, 1, 1, 1, 1, 1))
    x, z = paulis.codes_to_masks(paulis.terms_to_codes(labels, n))
    sv = DeviceSV(n)
    sv.apply(_lib.ops_array(device_ops(to_circuit(n, ref.brickwork(n, 8, 0)))))
    sv.pauli_expect_masks(x, z)
    svr = {"n": n, "terms": len(labels), "wall": stats([clock(lambda: sv.pauli_expect_masks(x, z))[0] for _ in range(reps)])}
    _lib.timing_enable(True)
    _lib.timing_reset()
    for _ in range(reps):
        sv.pauli_expect_masks(x, z)
    k = _lib.timing_query("sv_pauli")
    _lib.timing_enable(False)
    svr["kernels_ms"] = per(k)
    svr["bytes_per_call"] = k["bytes"] / max(k["launches"], 1)
    svr["achieved_bytes_per_s"] = svr["bytes_per_call"] / (svr["kernels_ms"] * 1e-3)
    res["statevector"] = svr

    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(res, f, indent=1)
    print(json.dumps(res))


if __name__ == "__main__":
    main()
