"""Two-site DMRG measurements -> profiles/dmrg.json, one MI355X.

The open antiferromagnetic Heisenberg chain (jx = jy = jz = -1):

- at --n (50) and --chi (64): calculate_ground_state_mps's loop driven by hand so that every sweep is timed
  on its own (DeviceDMRG.sweep ends in a device synchronise): energy, E / n, sigma^2, sweeps, wall time per
  sweep; then one more sweep under the HIP-event timers (aqc_timing_*): launches and kernel time per bond
  update for H_eff (dmrg_heff), the Krylov vector kernels (dmrg_krylov), the environment steps (dmrg_env)
  and the engine's theta / SVD / split, and H_eff's FLOP rate against the FP64 matrix ceiling.  The timed
  sweep runs on the converged state, where the bonds are full: its figures are those of a late sweep.
- at --small (24): the same chain through calculate_ground_state (the statevector Lanczos) and through
  calculate_ground_state_mps, side by side: both energies and both wall times.

Usage: python tools/dmrg_profile.py [--n 50] [--chi 64] [--small 24] [--out profiles/dmrg.json]
"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

FP64_PEAK_TFLOPS = 78.6  # the FP64 matrix rate the other profiles use
FAMILIES = ("dmrg_heff", "dmrg_krylov", "dmrg_env", "mps_theta", "mps_svd", "mps_split")


def large(n, chi, tol, max_sweeps, krylov_dim):
    from adaptaqc_amd import _lib, paulis
    from adaptaqc_amd.device import DeviceDMRG, DeviceMPS, dmrg_plan
    from adaptaqc_amd.utils import hamiltonians

    ham = hamiltonians.heisenberg_hamiltonian(n, -1.0, -1.0, -1.0)
    labels = list(ham)
    coeffs = np.array([ham[s] for s in labels])
    codes = paulis.terms_to_codes(labels, n)
    scale = float(np.sum(np.abs(coeffs)))
    plan = dmrg_plan(n, ham, chi_cap=chi, krylov_dim=krylov_dim)
    mps = DeviceMPS(n, chi, 1e-16, chi)
    rng = np.random.default_rng(0)
    ops = []
    for q in range(n):  # calculate_ground_state_mps's default start
        t, p = rng.uniform(0.0, np.pi), rng.uniform(0.0, 2.0 * np.pi)
        ry = np.array([[np.cos(t / 2), -np.sin(t / 2)], [np.sin(t / 2), np.cos(t / 2)]], dtype=complex)
        ops.append((np.diag([np.exp(-0.5j * p), np.exp(0.5j * p)]) @ ry, (q,)))
    mps.apply(ops)
    dm = DeviceDMRG(mps, ham, krylov_dim)
    energies, sweep_ms = [], []
    converged = False
    for _ in range(max_sweeps):
        t0 = time.perf_counter()
        dm.sweep()
        sweep_ms.append((time.perf_counter() - t0) * 1e3)
        energies.append(float(np.dot(coeffs, mps.pauli_expect(codes))))
        print(f"n={n} sweep {len(energies)}: E {energies[-1]!r} in {sweep_ms[-1]:.1f} ms, max bond {int(mps.dims().max())}",
              flush=True)
        if len(energies) > 1 and abs(energies[-1] - energies[-2]) <= tol * scale:
            converged = True
            break
    t0 = time.perf_counter()
    sq_codes, sq_coeffs = hamiltonians._squared_operator(codes, coeffs)
    host_ms = (time.perf_counter() - t0) * 1e3
    t0 = time.perf_counter()
    variance = float(np.dot(sq_coeffs, mps.pauli_expect(sq_codes))) - energies[-1] ** 2
    var_ms = (time.perf_counter() - t0) * 1e3
    # one more sweep under the event timers
    updates = 2 * (n - 1)
    _lib.timing_enable(True)
    _lib.timing_reset()
    t0 = time.perf_counter()
    dm.sweep()
    timed_ms = (time.perf_counter() - t0) * 1e3
    fam = {f: _lib.timing_query(f) for f in FAMILIES}
    _lib.timing_enable(False)
    per_bond = {f: {"launch_groups_per_bond": q["launches"] / updates, "kernel_ms_per_bond": q["ms"] / updates}
                for f, q in fam.items()}
    heff = fam["dmrg_heff"]
    heff_tflops = heff["flops"] / (heff["ms"] * 1e-3) / 1e12 if heff["ms"] > 0 else 0.0
    stats = dm.stats()
    out = {
        "n": n, "chi": chi, "krylov_dim": krylov_dim, "tol": tol, "terms": len(labels), "scale": scale,
        "converged": converged, "sweeps": len(energies), "energies": energies, "energy": energies[-1],
        "energy_per_site": energies[-1] / n, "variance": variance, "variance_resolution": 1e-11 * scale ** 2,
        "variance_terms": int(len(sq_codes)), "variance_host_ms": host_ms, "variance_device_ms": var_ms,
        "max_bond": int(mps.dims().max()), "sweep_wall_ms": sweep_ms, "sweep_wall_ms_last": sweep_ms[-1],
        "timed_sweep_wall_ms": timed_ms, "bond_updates_per_sweep": updates,
        # launches per bond update: 2 per H_eff apply (stage one, stage two), krylov_dim applies; the Krylov
        # kernels: init, krylov_dim steps, solve, combine; one environment step; theta, SVD, rank, 2 split
        "launches_per_bond": {"dmrg_heff": 2 * krylov_dim, "dmrg_krylov": krylov_dim + 3, "dmrg_env": 1,
                              "engine": 5},
        "per_bond": per_bond,
        "heff_flops_per_sweep": heff["flops"], "heff_kernel_ms_per_sweep": heff["ms"],
        "heff_tflops": heff_tflops, "fp64_matrix_peak_tflops": FP64_PEAK_TFLOPS,
        "heff_share_of_fp64_peak": heff_tflops / FP64_PEAK_TFLOPS,
        "breakdowns": stats["breakdowns"], "updates": stats["updates"],
        "plan": {k: plan[k] for k in ("total_records", "max_records", "env_matrices", "env_bytes", "scratch_bytes")},
    }
    dm.close()
    mps.close()
    return out


def small(n, chi, tol):
    from adaptaqc_amd.utils import hamiltonians

    ham = hamiltonians.heisenberg_hamiltonian(n, -1.0, -1.0, -1.0)
    out = {"n": n, "chi": chi, "tol": tol}
    for rep in range(2):  # the second pass is the warm one
        t0 = time.perf_counter()
        e_sv, psi = hamiltonians.calculate_ground_state(ham, tol=tol, return_device=True)
        sv_s = time.perf_counter() - t0
        psi.close()
        run = hamiltonians.last_run
        t0 = time.perf_counter()
        e_mps, mps = hamiltonians.calculate_ground_state_mps(ham, max_chi=chi, tol=tol, return_device=True)
        mps_s = time.perf_counter() - t0
        mps.close()
        mrun = hamiltonians.last_run_mps
        out["first" if rep == 0 else "warm"] = {
            "statevector": {"energy": e_sv, "wall_s": sv_s, "iterations": run.iterations, "restarts": run.restarts,
                            "residual": run.residual},
            "mps": {"energy": e_mps, "wall_s": mps_s, "sweeps": mrun.sweeps, "max_bond": mrun.max_bond,
                    "variance": mrun.variance},
            "energy_difference": e_mps - e_sv,
        }
        print(f"n={n} pass {rep}: statevector {e_sv!r} in {sv_s:.3f} s, DMRG {e_mps!r} in {mps_s:.3f} s", flush=True)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=50)
    ap.add_argument("--chi", type=int, default=64)
    ap.add_argument("--small", type=int, default=24)
    ap.add_argument("--tol", type=float, default=1e-9)
    ap.add_argument("--max-sweeps", type=int, default=30)
    ap.add_argument("--krylov-dim", type=int, default=6)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "dmrg.json"))
    args = ap.parse_args()
    res = {"hamiltonian": "open Heisenberg chain, jx = jy = jz = -1"}
    res["large"] = large(args.n, args.chi, args.tol, args.max_sweeps, args.krylov_dim)
    if args.small:
        res["small"] = small(args.small, args.chi, args.tol)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(res, f, indent=1, default=lambda o: o.tolist())  # (numpy scalars and arrays)
    print(json.dumps({k: res["large"][k] for k in ("energy", "energy_per_site", "variance", "sweeps", "sweep_wall_ms_last",
                                                     "heff_tflops")}))


if __name__ == "__main__":
    main()
