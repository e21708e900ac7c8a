"""Noisy pair tomography on the MPS engine, the host side (no GPU): aqc_mps_traj_pair_tomo's schedule
(aqc_mps_traj_tomo_plan) replayed in numpy on Vidal tensors and read out by full contraction, the dense
restatement (mps_traj_tomography_ref.py) against the density matrix, and QiskitSamplingBackend's routing."""
import itertools

import numpy as np
import pytest

import mps_traj_tomography_ref as mtref
import sampling_ref as ref
import tomography_ref as tomo
import traj_tomography_ref as ttref
from conftest import to_circuit


# ---- the schedule replayed on Vidal tensors -------------------------------------------------------
def _replay(n, sched, u):
    """One trajectory of the schedule on Vidal tensors, as test_mps_trajectory_host._replay runs it (theta,
    numpy.linalg.svd, lambda division; sigma^2 <= 1e-16 chopped; a Kraus row by the local rho formula):
    (gam, lam, choices by event)."""
    from adaptaqc_amd import _lib

    gam = [np.zeros((2, 1, 1), dtype=complex) for _ in range(n)]
    for g in gam:
        g[0, 0, 0] = 1.0
    lam = [np.ones(1) for _ in range(n + 1)]
    choices = {}
    for row in sched:
        p, flags = int(row["q0"]), int(row["flags"])
        m = np.asarray(row["m"]).view(np.complex128)
        if flags == 0 and int(row["nq"]) == 2:
            g4 = m[:16].reshape(2, 2, 2, 2)  # [s1', s2', s1, s2]
            a = lam[p][None, :, None] * gam[p] * lam[p + 1][None, None, :]
            b = gam[p + 1] * lam[p + 2][None, None, :]
            theta = np.einsum("abst,slm,tmr->albr", g4, a, b)
            cl, cr = theta.shape[1], theta.shape[3]
            uu, s, vh = np.linalg.svd(theta.reshape(2 * cl, 2 * cr), full_matrices=False)
            keep = max(1, int(np.count_nonzero(s ** 2 > 1e-16)))
            uu, s, vh = uu[:, :keep], s[:keep], vh[:keep]
            lam[p + 1] = s / np.linalg.norm(s)
            gam[p] = uu.reshape(2, cl, keep) / lam[p][None, :, None]
            gam[p + 1] = vh.reshape(keep, 2, cr).transpose(1, 0, 2) / lam[p + 2][None, None, :]
        elif flags == 0:
            gam[p] = np.einsum("st,tlr->slr", m[:4].reshape(2, 2), gam[p])
        else:
            assert flags & 0xFF == _lib.OP_KRAUS1, "a measurement row in the readout's schedule"
            event, nk = flags >> 8, int(row["q1"])
            ks = [m[4 * k: 4 * k + 4].reshape(2, 2) for k in range(nk)]
            w = (lam[p] ** 2)[:, None] * (lam[p + 1] ** 2)[None, :]
            rho = np.einsum("lr,slr,tlr->st", w, gam[p], gam[p].conj())
            pk = np.array([max(0.0, float(np.real(np.trace(k.conj().T @ k @ rho)))) for k in ks])
            c = np.cumsum(pk)
            above = np.flatnonzero(c > u[event] * c[-1])
            k = int(above[0]) if above.size else int(np.flatnonzero(pk > 0)[-1])
            choices[event] = k
            gam[p] = np.einsum("st,tlr->slr", ks[k] / np.sqrt(pk[k]), gam[p])
    return gam, lam, choices


def _contracted_pair_rdm(gam, lam, hi, lo):
    """The 4x4 RDM (index 2 bit_hi + bit_lo) of sites (hi, lo) by full contraction of <psi| and |psi>
    site by site, A_j = lambda_j Gamma_j: no canonical form assumed."""
    env = np.ones((1, 1), dtype=complex)  # [open indices ..., ket bond, bra bond]
    for j, g in enumerate(gam):
        a = lam[j][None, :, None] * g  # [s, l, r]
        if j in (hi, lo):
            env = np.einsum("...ab,sac,tbd->...stcd", env, a, a.conj())
        else:
            env = np.einsum("...ab,sac,sbd->...cd", env, a, a.conj())
    r = env[..., 0, 0]  # [s_lo, t_lo, s_hi, t_hi]
    return np.einsum("ltLT->LlTt", r).reshape(4, 4)


# (n, ops): a non-adjacent cx whose routing leaves the qubits unsorted before the final sort, a rotation
# pending on a qubit when its Kraus row arrives, and gates without an error (h, x) pending at the end: the
# flush's one-site rows
REPLAY_CASES = [
    (5, [("ry", (0,), (0.9,)), ("rx", (3,), (0.4,)), ("cx", (0, 3), ()), ("rz", (2,), (1.3,)), ("cx", (4, 1), ()),
         ("ry", (1,), (0.7,)), ("cx", (1, 2), ()), ("rx", (4,), (1.1,)), ("h", (2,), ()), ("x", (0,), ())]),
    (6, ref.brickwork(6, 2, 31) + [("cx", (5, 1), ()), ("ry", (3,), (0.6,)), ("cx", (0, 4), ()), ("h", (4,), ())]),
]


@pytest.mark.parametrize("t2", [70e3, 30e3])
@pytest.mark.parametrize("n,ops", REPLAY_CASES)
def test_readout_schedule_replayed_on_vidal_tensors(n, ops, t2):
    """The schedule of the pair readout -- no measurement row; it ends with the flush and the sort --
    replayed on Vidal tensors: the Kraus choices are the dense restatement's, and after the last row the
    full contraction of every pair's RDM from (Gamma, lambda) equals the dense trajectory state's to
    1e-10, for t2 on both sides of t1."""
    from adaptaqc_amd import _lib
    from adaptaqc_amd.device import mps_trajectory_plan
    from adaptaqc_amd.noise import trajectory_program

    rows, n_events, _ = trajectory_program(to_circuit(n, ops), ttref.model(t2, readout=False))
    counts, sched = mps_trajectory_plan(n, rows, return_schedule=True, measure=False)
    full, full_sched = mps_trajectory_plan(n, rows, return_schedule=True)
    assert counts["measure_rows"] == 0 and counts["kraus_rows"] == n_events > 0
    assert counts["one_site_rows"] >= 1 and counts["swap_updates"] >= 1 and counts["centre_moves"] >= 1
    # the sampler's schedule is this one followed by its measurement sweep
    assert full["measure_rows"] == n and full["rows"] > counts["rows"]
    assert sched.tobytes() == full_sched[:len(sched)].tobytes()
    assert not np.any(sched["flags"] == _lib.OP_MEASURE1)
    for key in ("gate_updates", "swap_updates", "one_site_rows", "kraus_rows"):
        assert counts[key] == full[key]
    shots = 6
    pairs = tomo.all_pairs(n)
    u = ref.uniforms(78 + n, 0, shots, n_events)
    psi, want_k, near, _ = mtref.evolve(n, rows, u)
    assert not near.any()
    worst = 0.0
    for s in range(shots):
        gam, lam, choices = _replay(n, sched, u[s])
        assert [choices[e] for e in range(n_events)] == list(want_k[s]), s
        for a, b in pairs:
            hi, lo = max(a, b), min(a, b)
            want = ttref.pair_rdms(psi[s:s + 1], n, hi, lo)[0]
            worst = max(worst, float(np.max(np.abs(_contracted_pair_rdm(gam, lam, hi, lo) - want))))
    print(f"n={n} t2={t2:g}: {counts}, contracted pair RDMs off by at most {worst:.2e}")
    assert worst < 1e-10


def test_kraus_branches_of_the_restatement_sum_to_the_exact_tables():
    """Two Kraus events on two qubits: the restatement's per-trajectory probabilities, weighted over every
    sequence of Kraus choices, are the density matrix's (traj_tomography_ref.exact_tables).  The uniforms
    0 and just below 1 steer a two-operator event to its first and its last operator."""
    from adaptaqc_amd import noise
    from adaptaqc_amd.circuit import QuantumCircuit

    qc = QuantumCircuit(2)
    qc.ry(0.8, 0)
    qc.cx(0, 1)
    nm = ttref.model()
    rows, n_events, _ = noise.trajectory_program(qc, nm)
    rows = rows[:-1]  # two events: drop the last Kraus row (on the cx's second qubit)
    kraus = rows[rows["flags"] == 1]
    assert len(kraus) == 2
    nks = [int(k) for k in kraus["q1"]]
    effects = noise.readout_effects(2, nm)
    pairs = [(1, 0)]
    want = ttref.exact_tables(2, rows, pairs, effects)
    # one block of nine trajectories (one per setting) per sequence of choices; event e takes operator
    # k for u just above C_{k-1} / P, which the restatement itself reports
    got = np.zeros_like(want)
    total = 0.0
    for seq in itertools.product(*[range(k) for k in nks]):
        u = np.zeros((9, 2))
        weight = 1.0
        for e, k in enumerate(seq):
            # the branch's conditional probabilities at event e, from a trial evolution up to it
            probs = _event_probs(2, rows, u[:1], e)
            if probs[k] <= 0:
                weight = 0.0
                break
            u[:, e] = (np.sum(probs[:k]) + 0.5 * probs[k]) / np.sum(probs)
            weight *= probs[k] / np.sum(probs)
        if weight == 0.0:
            continue
        p, near, n_ev = mtref.trajectory_probs(2, rows, pairs, effects, u)
        assert n_ev == 2 and not near.any()
        got[0] += weight * p[0]
        total += weight
    assert abs(total - 1) < 1e-12
    assert np.max(np.abs(got - want)) < 1e-12
    # and the restatement's shots follow that law
    shots = 2000
    u = ref.uniforms(3, 0, 9 * shots, 2 + 1)
    outcomes, counts, near = mtref.pair_tomography(2, rows, pairs, effects, u)
    assert counts.sum(axis=2).tolist() == [[shots] * 9] and near.sum() <= 1
    assert np.array_equal(counts, ttref.counts_of(outcomes))
    assert np.max(np.abs(counts[0] / shots - want[0])) < 6 * 0.5 / np.sqrt(shots)
    # away from the bands it is traj_tomography_ref's restatement, outcome by outcome
    sv_outcomes, _, sv_near = ttref.pair_tomography(2, rows, pairs, effects, u)
    assert not sv_near.any() and np.array_equal(outcomes[~near], sv_outcomes[~near])


def _event_probs(n, rows, u, event):
    """p_k of Kraus event ``event`` of the trajectory that follows u [1, >= event] before it."""
    import trajectory_ref as tref

    upto = int(np.flatnonzero(rows["flags"] == tref.KRAUS1)[event])
    psi = mtref.evolve(n, rows[:upto], u)[0]
    row = rows[upto]
    return np.array([float(np.sum(np.abs(tref.apply(psi, n, k, (int(row["q0"]),))) ** 2)) for k in tref._matrices(row)])


# ---- the backend's routing ------------------------------------------------------------------------
class _Recorder:
    """Stands in for device.mps_trajectory_pair_tomography: records the calls, fails the first ``fail``
    of them with the engine's capacity error, and returns uniform tables."""

    def __init__(self, fail=0):
        self.calls, self.fail = [], fail

    def __call__(self, n, rows, n_events, pairs, effects, shots, seed, run=0, u=None, return_outcomes=False,
                 chi_cap=64, threshold=1e-16, max_chi=None):
        from adaptaqc_amd._lib import AqcError

        self.calls.append(dict(n=n, n_events=n_events, pairs=list(pairs), shots=shots, seed=seed, run=run,
                               chi_cap=chi_cap, threshold=threshold, max_chi=max_chi, effects=np.array(effects)))
        if len(self.calls) <= self.fail:
            raise AqcError("rc=-3: MPS bond capacity (chi_cap) exceeded: increase chi_cap or set max_chi")
        return np.full((len(pairs), 9, 4), shots // 4, dtype=np.int64)


def _no_gpu(monkeypatch, recorder):
    """The device calls of the noisy MPS route replaced: the recorder, and a fit that needs no GPU."""
    from adaptaqc_amd import device

    monkeypatch.setattr(device, "mps_trajectory_pair_tomography", recorder)
    monkeypatch.setattr(device, "tomo_fit", lambda counts: np.zeros((len(counts), 4, 4), dtype=complex))

    def refuse(*a, **k):
        raise AssertionError("the statevector entry was called")

    monkeypatch.setattr(device, "trajectory_pair_tomography", refuse)


def _wide_circuit(n):
    return to_circuit(n, [("rx", (0,), (0.3,)), ("cx", (0, n - 1), ())])


def test_backend_routes_to_the_mps_entry(monkeypatch):
    from adaptaqc_amd import mps_operations as mops
    from adaptaqc_amd.backends.qiskit_sampling_backend import QiskitSamplingBackend, SamplingSimulator
    from adaptaqc_amd.noise import readout_effects, trajectory_program

    nm = ttref.model()
    for method, n in (("matrix_product_state", 4), ("automatic", 26)):
        rec = _Recorder()
        _no_gpu(monkeypatch, rec)
        sim = SamplingSimulator(method=method, seed=5, mps_trajectories=True, mps_truncation_threshold=1e-12)
        be = QiskitSamplingBackend(sim, tomography="device", trajectory_tomography=True)
        qc = _wide_circuit(n)
        qc.measure(0, 0)  # tomography strips the classical operations
        rho, vals = be.pair_tomography(qc, [(0, n - 1), (2, 1)], {"shots": 64, "noise_model": nm, "seed_simulator": 7})
        assert rho.shape == (2, 4, 4) and vals is None
        (call,) = rec.calls
        rows, n_events, _ = trajectory_program(_wide_circuit(n), nm)
        assert call["n"] == n and call["n_events"] == n_events > 0 and call["pairs"] == [(0, n - 1), (2, 1)]
        assert (call["shots"], call["seed"], call["run"]) == (64, 7, 0)
        assert call["chi_cap"] == mops.chi_cap_for(n, None, 1, {}) and call["threshold"] == 1e-12 and call["max_chi"] is None
        assert np.array_equal(call["effects"], readout_effects(n, nm))
        # without seed_simulator: the simulator's seed and its run counter, advanced once per sweep
        be.pair_tomography(qc, [(0, 1)], {"shots": 64, "noise_model": nm})
        be.pair_tomography(qc, [(0, 1)], {"shots": 64, "noise_model": nm})
        assert [(c["seed"], c["run"]) for c in rec.calls[1:]] == [(5, 0), (5, 1)] and sim.runs == 2
    # automatic up to 24 qubits stays on the statevector entry, with or without the flag
    calls = []
    rec = _Recorder()
    _no_gpu(monkeypatch, rec)
    from adaptaqc_amd import device
    monkeypatch.setattr(device, "trajectory_pair_tomography",
                        lambda n, *a, **k: calls.append(n) or np.zeros((1, 9, 4), dtype=np.int64))
    be = QiskitSamplingBackend(SamplingSimulator(mps_trajectories=True), tomography="device", trajectory_tomography=True)
    be.pair_tomography(_wide_circuit(4), [(0, 1)], {"shots": 64, "noise_model": nm})
    assert calls == [4] and rec.calls == []
    # a bounded run passes max_chi on as the capacity
    rec = _Recorder()
    _no_gpu(monkeypatch, rec)
    sim = SamplingSimulator(method="matrix_product_state", mps_trajectories=True, max_chi=8)
    QiskitSamplingBackend(sim, tomography="device", trajectory_tomography=True).pair_tomography(
        _wide_circuit(6), [(0, 1)], {"shots": 64, "noise_model": nm})
    assert (rec.calls[0]["chi_cap"], rec.calls[0]["max_chi"]) == (8, 8)


def test_backend_grows_the_capacity_and_repeats_the_same_trajectories(monkeypatch):
    from adaptaqc_amd import mps_operations as mops
    from adaptaqc_amd._lib import AqcError
    from adaptaqc_amd.backends.qiskit_sampling_backend import QiskitSamplingBackend, SamplingSimulator

    nm = ttref.model()
    n = 26
    rec = _Recorder(fail=1)
    _no_gpu(monkeypatch, rec)
    sim = SamplingSimulator(method="automatic", seed=11, mps_trajectories=True)
    be = QiskitSamplingBackend(sim, tomography="device", trajectory_tomography=True)
    be.pair_tomography(_wide_circuit(n), [(0, 25)], {"shots": 32, "noise_model": nm})
    first, second = rec.calls
    assert first["chi_cap"] == mops.chi_cap_for(n, None, 1, {}) and second["chi_cap"] == 2 * first["chi_cap"]
    assert (first["seed"], first["run"]) == (second["seed"], second["run"]) == (11, 0) and sim.runs == 1
    # the capacity is learned: the next sweep starts there
    be.pair_tomography(_wide_circuit(n), [(0, 25)], {"shots": 32, "noise_model": nm})
    assert rec.calls[2]["chi_cap"] == second["chi_cap"] and rec.calls[2]["run"] == 1
    # a bounded run cannot grow: the error comes through; so does any other error
    rec = _Recorder(fail=1)
    _no_gpu(monkeypatch, rec)
    bounded = SamplingSimulator(method="matrix_product_state", mps_trajectories=True, max_chi=4)
    with pytest.raises(AqcError, match="capacity"):
        QiskitSamplingBackend(bounded, tomography="device", trajectory_tomography=True).pair_tomography(
            _wide_circuit(6), [(0, 1)], {"shots": 32, "noise_model": nm})
    assert len(rec.calls) == 1


def test_backend_refusals_keep_their_messages(monkeypatch):
    from adaptaqc_amd.backends.qiskit_sampling_backend import QiskitSamplingBackend, SamplingSimulator

    rec = _Recorder()
    _no_gpu(monkeypatch, rec)
    nm = ttref.model()
    kwargs = {"shots": 50, "noise_model": nm}
    be = QiskitSamplingBackend(SamplingSimulator(method="matrix_product_state"), tomography="device",
                               trajectory_tomography=True)
    with pytest.raises(NotImplementedError, match="matrix_product_state") as err:
        be.pair_tomography(_wide_circuit(4), [(0, 1)], kwargs)
    assert "mps_trajectories=True" in str(err.value)
    be = QiskitSamplingBackend(SamplingSimulator(method="automatic"), tomography="device", trajectory_tomography=True)
    with pytest.raises(NotImplementedError, match="24 qubits") as err:
        be.pair_tomography(_wide_circuit(26), [(0, 1)], kwargs)
    assert "mps_trajectories=True" in str(err.value)
    # statevector above 24 qubits raises whatever the flag
    for flag in (False, True):
        be = QiskitSamplingBackend(SamplingSimulator(method="statevector", mps_trajectories=flag), tomography="device",
                                   trajectory_tomography=True)
        with pytest.raises(NotImplementedError, match="24 qubits"):
            be.pair_tomography(_wide_circuit(26), [(0, 1)], kwargs)
    # the concurrence lower bound under a model, and the backend without the flag, refuse as before
    mps = QiskitSamplingBackend(SamplingSimulator(method="matrix_product_state", mps_trajectories=True),
                                tomography="device", trajectory_tomography=True)
    with pytest.raises(NotImplementedError, match="noise_model"):
        mps.concurrence_lower_bounds(_wide_circuit(4), [(0, 1)], kwargs)
    plain = QiskitSamplingBackend(SamplingSimulator(method="matrix_product_state", mps_trajectories=True),
                                  tomography="device")
    with pytest.raises(NotImplementedError, match="noise_model"):
        plain.pair_tomography(_wide_circuit(4), [(0, 1)], kwargs)
    assert rec.calls == []
