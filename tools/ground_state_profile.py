"""Ground-state measurements -> profiles/ground_state.json.

Heisenberg chains (jx = jy = jz = -1, open) at n = 16, 20, 24, on a random normalised state:

- DeviceSV.pauli_apply (aqc_sv_pauli_apply): wall time and HIP-event kernel time, beside
  DeviceSV.pauli_expect (aqc_sv_pauli_expect) on the same terms and state in the same process -- the
  expectation reads two amplitudes per term, the apply one per group and writes one;
- the apply's share of the 6.29 TB/s copy rate on (groups + 2) 16 2^n bytes (one read of the state
  per group, one more for the first touch, one write);
- DeviceSV.dot and DeviceSV.axpby, the other two calls of a Lanczos step;
- calculate_ground_state at tol = 1e-9: Lanczos steps, restarts, residual and wall time.

Usage: python tools/ground_state_profile.py [--sizes 16 20 24] [--reps 5] [--out profiles/ground_state.json]
"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

COPY_RATE_TBS = 6.29  # the measured device copy rate the README quotes


def timed(fn, reps):
    fn()
    ts = []
    for _ in range(reps):
        t0 = time.perf_counter()
        fn()
        ts.append((time.perf_counter() - t0) * 1e3)
    return {"median_ms": float(np.median(ts)), "min_ms": float(np.min(ts)), "reps": reps}


def kernel_ms(_lib, family, fn, reps):
    _lib.timing_enable(True)
    _lib.timing_reset()
    for _ in range(reps):
        fn()
    q = _lib.timing_query(family)
    _lib.timing_enable(False)
    return q["ms"] / max(q["launches"], 1)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sizes", type=int, nargs="+", default=[16, 20, 24])
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "ground_state.json"))
    args = ap.parse_args()

    from adaptaqc_amd import _lib, paulis
    from adaptaqc_amd.device import DeviceSV
    from adaptaqc_amd.utils import hamiltonians

    res = {"copy_rate_tbs": COPY_RATE_TBS, "hamiltonian": "open Heisenberg chain, jx = jy = jz = -1", "sizes": []}
    for n in args.sizes:
        ham = hamiltonians.heisenberg_hamiltonian(n, -1.0, -1.0, -1.0)
        labels = list(ham)
        x, z, c = paulis.operator_to_masks(ham, n)
        groups = len(paulis.group_by_xmask(x, z, c))
        rng = np.random.default_rng(n)
        psi = rng.normal(size=1 << n) + 1j * rng.normal(size=1 << n)
        psi /= np.linalg.norm(psi)
        a, b = DeviceSV(n), DeviceSV(n)
        a.set(psi)
        del psi
        row = {"n": n, "terms": len(labels), "groups": groups}
        row["pauli_apply_wall"] = timed(lambda: a.pauli_apply_masks(x, z, c, b), args.reps)
        row["pauli_apply_kernel_ms"] = kernel_ms(_lib, "sv_pauli_apply", lambda: a.pauli_apply_masks(x, z, c, b), args.reps)
        row["pauli_expect_wall"] = timed(lambda: a.pauli_expect_masks(x, z), args.reps)
        row["pauli_expect_kernel_ms"] = kernel_ms(_lib, "sv_pauli", lambda: a.pauli_expect_masks(x, z), args.reps)
        row["apply_over_expect_kernel"] = row["pauli_apply_kernel_ms"] / row["pauli_expect_kernel_ms"]
        nbytes = (groups + 2) * 16.0 * 2.0 ** n
        row["apply_bytes"] = nbytes
        row["apply_tbs"] = nbytes / (row["pauli_apply_kernel_ms"] * 1e-3) / 1e12
        row["apply_share_of_copy_rate"] = row["apply_tbs"] / COPY_RATE_TBS
        row["dot_wall"] = timed(lambda: a.dot(b), args.reps)
        row["dot_kernel_ms"] = kernel_ms(_lib, "sv_dot", lambda: a.dot(b), args.reps)
        row["axpby_wall"] = timed(lambda: b.axpby(1.0, a, 1e-3), args.reps)
        row["axpby_kernel_ms"] = kernel_ms(_lib, "sv_axpby", lambda: b.axpby(1.0, a, 1e-3), args.reps)
        a.close()
        b.close()
        t0 = time.perf_counter()
        energy, dev = hamiltonians.calculate_ground_state(ham, tol=1e-9, return_device=True)
        wall = time.perf_counter() - t0
        dev.close()
        run = hamiltonians.last_run
        row["ground_state"] = {"tol": 1e-9, "energy": energy, "energy_per_site": energy / n, "residual": run.residual,
                               "tol_times_S": 1e-9 * run.scale, "lanczos_steps": run.iterations,
                               "restarts": run.restarts, "wall_s": wall}
        res["sizes"].append(row)
        print(json.dumps(row), flush=True)

    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(res, f, indent=1)
    print(json.dumps(res))


if __name__ == "__main__":
    main()
