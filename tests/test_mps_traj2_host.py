"""The host side of correlated two-qubit groups on the MPS trajectory engine (csrc/mps_traj.hip):
aqc_mps_traj_set_correlated and the keywords above it, the planner's two group paths replayed on a dense
state against trajectory2_ref, the centre bookkeeping at every two-site row and general group, and the
malformed groups.  No GPU."""
import ctypes

import numpy as np
import pytest

import sampling_ref as ref
import trajectory2_ref as t2ref
from adaptaqc_amd import _lib, gates, noise
from trajectory_ref import apply

PRODUCT = 1 << 24  # a product-unitary group's rows in the plan


@pytest.fixture
def mode():
    """Sets the engine's process-wide switch and restores 0 afterwards."""
    lib = _lib.load()  # (does not touch the GPU)

    def set_mode(m):
        return lib.aqc_mps_traj_set_correlated(m)

    yield set_mode
    assert lib.aqc_mps_traj_set_correlated(0) == 0


def _plan(n, rows, correlated=1, measure=True):
    from adaptaqc_amd.device import mps_trajectory_plan

    return mps_trajectory_plan(n, rows, return_schedule=True, measure=measure, correlated=correlated)


def _is_group(sched):
    return (sched["flags"] & 0xFF) == _lib.OP_KRAUS2


# ---- the setter and the keywords --------------------------------------------------------------------
def test_setter_range_and_symbol(mode):
    assert "aqc_mps_traj_set_correlated" in _lib.EXPORTS
    import os

    header = open(os.path.join(os.path.dirname(_lib.__file__), "..", "include", "aqc_hip.h")).read()
    assert "int aqc_mps_traj_set_correlated(int mode);" in header
    for ok in (0, 1, 2, 0):
        assert mode(ok) == 0
    for bad in (-1, 3, 1 << 20):
        assert mode(bad) == -1
    assert mode(0) == 0


def test_keyword_validation():
    from adaptaqc_amd.backends.qiskit_sampling_backend import SamplingSimulator
    from adaptaqc_amd.device import mps_trajectory_plan

    with pytest.raises(ValueError, match="mps_correlated"):
        SamplingSimulator(mps_correlated=True)
    with pytest.raises(ValueError, match="mps_correlated"):
        SamplingSimulator(method="matrix_product_state", mps_pauli_readout=False, mps_correlated=True)
    sim = SamplingSimulator(method="matrix_product_state", mps_trajectories=True, mps_correlated=True)
    assert sim.mps_correlated is True
    old = SamplingSimulator(method="matrix_product_state", mps_trajectories=True)
    del old.__dict__["mps_correlated"]  # a pickle from before the flag
    _, rows, _ = t2ref.program(3, 1, "a")
    with pytest.raises(NotImplementedError, match="correlated.*24 qubits"):
        old._refuse_correlated_on_mps(rows)
    sim._refuse_correlated_on_mps(rows)  # the flag lifts the refusal
    assert "mps_correlated=True" in noise._CORRELATED_ON_MPS and "correlated=True" in noise._CORRELATED_ON_MPS
    with pytest.raises(ValueError):
        mps_trajectory_plan(3, rows, correlated=3)


@pytest.mark.parametrize("which", ["a", "b", "c"])
def test_mode_zero_refuses_and_mode_one_plans(mode, which):
    _, rows, n_events = t2ref.program(3, 1, which)
    rows = np.ascontiguousarray(rows)
    lib = _lib.load()
    counts = np.zeros(7, dtype=np.int32)
    for entry in (lib.aqc_mps_traj_plan, lib.aqc_mps_traj_tomo_plan):
        assert mode(0) == 0
        assert entry(3, _lib.ptr(rows), len(rows), _lib.ptr(counts), None, 0) == -1
        assert mode(1) == 0
        assert entry(3, _lib.ptr(rows), len(rows), _lib.ptr(counts), None, 0) == 0
        assert counts[4] == n_events  # one event per group
    assert mode(0) == 0
    out = np.zeros((4, 1), dtype=np.uint64)
    assert lib.aqc_mps_traj_sample(3, 8, 1e-16, 0, _lib.ptr(rows), len(rows), 4, ctypes.c_uint64(1), ctypes.c_uint64(0),
                                   None, _lib.ptr(out), None) == -1


def test_the_wrapper_restores_the_refusal():
    """mps_trajectory_plan(correlated=True) sets the mode for the call only, also when the call fails."""
    from adaptaqc_amd._lib import AqcError
    from adaptaqc_amd.device import mps_trajectory_plan

    _, rows, n_events = t2ref.program(3, 1, "b")
    assert mps_trajectory_plan(3, rows, correlated=True)["kraus_rows"] == n_events
    counts = np.zeros(7, dtype=np.int32)
    r = np.ascontiguousarray(rows)
    assert _lib.load().aqc_mps_traj_plan(3, _lib.ptr(r), len(r), _lib.ptr(counts), None, 0) == -1
    bad = rows.copy()
    bad["q1"][int(np.flatnonzero(_is_group(bad))[0])] = 7
    with pytest.raises(AqcError, match="-1"):
        mps_trajectory_plan(3, bad, correlated=True)
    assert _lib.load().aqc_mps_traj_plan(3, _lib.ptr(r), len(r), _lib.ptr(counts), None, 0) == -1
    with pytest.raises(NotImplementedError, match="correlated.*24 qubits"):
        mps_trajectory_plan(3, rows)


# ---- the schedule replayed on a dense state -------------------------------------------------------------
def _choose(p, u):
    c = np.cumsum(p)
    above = np.flatnonzero(c > u * c[-1])
    return int(above[0]) if above.size else int(np.flatnonzero(p > 0)[-1])


def _replay(n, sched, u):
    """One shot of a plan without the measurement sweep on a dense state indexed by SITE (bit p = site
    p): every row acts on the sites it names with the matrix it carries, the routing and sorting swaps
    included, so the site <-> qubit map is followed by the state itself, and behind the final sort site
    p is qubit p again.  Returns (psi [2^n], choices)."""
    psi = np.zeros((1, 2 ** n), dtype=complex)
    psi[0, 0] = 1.0
    choices = []
    i = 0
    while i < len(sched):
        row = sched[i]
        p, q1, flags, nq = int(row["q0"]), int(row["q1"]), int(row["flags"]), int(row["nq"])
        m = np.asarray(row["m"]).view(np.complex128)
        if flags == 0 and nq == 2:
            assert q1 == p + 1
            psi = apply(psi, n, m.reshape(4, 4), (p + 1, p))  # index 2 s_p + s_{p+1}: site p the high bit
            i += 1
        elif flags == 0:
            psi = apply(psi, n, m[:4].reshape(2, 2), (p,))
            i += 1
        elif flags & 0xFF == _lib.OP_KRAUS1:
            assert flags >> 8 == len(choices)
            phis = [apply(psi, n, m[4 * k: 4 * k + 4].reshape(2, 2), (p,)) for k in range(q1)]
            pk = np.array([np.sum(np.abs(f) ** 2) for f in phis])
            k = _choose(pk, u[len(choices)])
            psi = phis[k] / np.sqrt(pk[k])
            choices.append(k)
            i += 1
        else:
            assert flags & 0xFF == _lib.OP_KRAUS2 and nq == 2 and p < q1
            nk = (flags >> 16) & 0xFF
            group = sched[i: i + nk]
            want = _lib.OP_KRAUS2 | (np.arange(nk) << 8) | (nk << 16) | (flags & PRODUCT)
            assert np.array_equal(group["flags"], want) and np.all(group["q0"] == p) and np.all(group["q1"] == q1)
            assert flags & PRODUCT or q1 == p + 1
            phis = [apply(psi, n, np.asarray(g["m"]).view(np.complex128).reshape(4, 4), (q1, p)) for g in group]
            pk = np.array([np.sum(np.abs(f) ** 2) for f in phis])
            k = _choose(pk, u[len(choices)])
            psi = phis[k] / np.sqrt(pk[k])
            choices.append(k)
            i += nk
    return psi[0], np.array(choices, dtype=np.uint8)


def _hand_built(listed):
    """5 qubits: pending rotations on qubits 0 and 3 (and one on 2 that no event meets), then a model-c
    group on the non-adjacent qubits ``listed`` with no gate before it, a cx across it and a second group."""
    err = t2ref.cx_error("c")
    ops = _lib.ops_array([(gates.one_qubit("ry", (0.9,)), (0,)), (gates.one_qubit("rx", (0.4,)), (3,)),
                          (gates.one_qubit("rz", (1.3,)), (2,))])
    cx = _lib.ops_array([(gates.two_qubit("cx"), (1, 3)), (gates.one_qubit("ry", (0.7,)), (3,))])
    return np.concatenate([ops, noise.kraus2_rows(err, listed), cx, noise.kraus2_rows(err, listed[::-1])])


def _replay_cases():
    cases = [(f"n={n} model {w}", n, t2ref.program(n, 2 if n > 2 else 1, w)[1]) for n in (2, 3, 4) for w in "abc"]
    cases.append(("hand-built (0, 3)", 5, _hand_built((0, 3))))
    cases.append(("hand-built (3, 0)", 5, _hand_built((3, 0))))
    return cases


REPLAY = _replay_cases()


@pytest.mark.parametrize("label,n,rows", REPLAY, ids=[c[0] for c in REPLAY])
@pytest.mark.parametrize("correlated", [1, 2])
def test_schedule_replayed_on_a_dense_state(label, n, rows, correlated):
    """The plan's rows (the schedule without the measurement sweep) on a dense state, shot by shot: the
    final states equal trajectory2_ref.evolve's within 1e-12 and the choices are equal -- routing,
    folding of pending gates, both orientations of the site order and both group paths."""
    n_events = noise.count_events(rows)
    counts, sched = _plan(n, rows, correlated, measure=False)
    assert counts["kraus_rows"] == n_events and counts["rows"] == len(sched) and counts["measure_rows"] == 0
    shots = 8
    u = ref.uniforms(123 + n, 0, shots, n_events)
    want_psi, want_k, near, _ = t2ref.evolve(n, rows, u)
    assert not near.any()
    worst = 0.0
    for s in range(shots):
        psi, choices = _replay(n, sched, u[s])
        assert np.array_equal(choices, want_k[s]), (label, s)
        worst = max(worst, float(np.max(np.abs(psi - want_psi[s]))))
    print(f"{label}, mode {correlated}: {counts}; states off by at most {worst:.2e}")
    assert worst < 1e-12


def test_hand_built_program_takes_both_orientations():
    """The two listings of the hand-built group fold the pending gates into different factors: the plans
    differ, and the first group is general with its qubits routed to adjacent sites."""
    a = _plan(5, _hand_built((0, 3)), measure=False)[1]
    b = _plan(5, _hand_built((3, 0)), measure=False)[1]
    ga, gb = a[_is_group(a)], b[_is_group(b)]
    assert len(ga) == len(gb) == 6 and not (ga["flags"] & PRODUCT).any()
    assert np.all(ga["q1"] == ga["q0"] + 1)
    assert not np.array_equal(ga["m"], gb["m"])
    # no one-site row in front of the first group: the pending rotations of qubits 0 and 3 went into it
    first = int(np.flatnonzero(_is_group(a))[0])
    assert not np.any((a["flags"][:first] == 0) & (a["nq"][:first] == 1))


# ---- the planner's invariants ------------------------------------------------------------------------
def _track(n, sched):
    """(a, b) by the planner's rules over the plan's rows; returns the number of rows whose precondition
    was checked (two-site rows and general groups), asserting it at each."""
    a, b = n, -1
    checked = 0
    i = 0
    while i < len(sched):
        row = sched[i]
        p, flags, nq = int(row["q0"]), int(row["flags"]), int(row["nq"])
        step = 1
        if flags & 0xFF == _lib.OP_KRAUS2:
            step = (flags >> 16) & 0xFF
        if flags == 0 and nq == 2:
            assert a >= p and b <= p + 1, (i, p, a, b)
            checked += 1
            a = a if a >= p + 2 else p + 1
            b = b if b <= p - 1 else p
        elif flags & 0xFF == _lib.OP_KRAUS2 and not flags & PRODUCT:
            # a general group: a two-site update's precondition; its operator is not unitary, so behind
            # it the centre stands on the two sites whatever was orthonormal before
            assert a >= p and b <= p + 1, (i, p, a, b)
            checked += 1
            a, b = p + 1, p
        elif flags & 0xFF == _lib.OP_KRAUS1 or flags == _lib.OP_MEASURE1:
            assert a >= p and b <= p, (i, p, a, b)
            a = b = p
        i += step
    return checked


def _two_site_rows(counts):
    return counts["gate_updates"] + counts["swap_updates"] + counts["centre_moves"]


@pytest.mark.parametrize("n,depth", [(3, 1), (4, 3), (6, 3)])
def test_planner_invariants(n, depth):
    for which in "abc":
        _, rows, n_events = t2ref.program(n, depth, which)
        for m in (1, 2):
            counts, sched = _plan(n, rows, m)
            assert _track(n, sched) >= _two_site_rows(counts) > 0
    _, rows, n_events = t2ref.program(n, depth, "a")
    counts, sched = _plan(n, rows, 1)
    groups = sched[_is_group(sched)]
    assert len(groups) > 0 and np.all(groups["flags"] & PRODUCT)  # model a: every group product-unitary
    # ... and no two-site row beyond those of the same program without its groups
    bare = rows[(rows["flags"] & 0xFF) != _lib.OP_KRAUS2]
    c0, _ = _plan(n, bare, 0)
    assert _two_site_rows(counts) == _two_site_rows(c0)
    assert counts["kraus_rows"] - c0["kraus_rows"] == len(groups) // 16
    # mode 2: the same groups on the general path, adjacent sites, each one more two-site update
    c2, s2 = _plan(n, rows, 2)
    g2 = s2[_is_group(s2)]
    assert len(g2) == len(groups) and not (g2["flags"] & PRODUCT).any() and np.all(g2["q1"] == g2["q0"] + 1)
    assert _track(n, s2) == _two_site_rows(c2) + len(g2) // 16
    assert c2["kraus_rows"] == counts["kraus_rows"] == n_events
    # models b and c are general under mode 1
    for which in "bc":
        s = _plan(n, t2ref.program(n, depth, which)[1], 1)[1]
        g = s[_is_group(s)]
        assert len(g) > 0 and not (g["flags"] & PRODUCT).any()


def test_a_product_group_moves_nothing():
    """cx(0, 3) on 5 qubits under model a, then a one-qubit error: the group's rows name the two sites the
    qubits sit on after the gate's routing, and the rows behind it are those of the program without it."""
    from conftest import to_circuit

    nm = noise.NoiseModel()
    nm.add_all_qubit_quantum_error(t2ref.cx_error("a"), "cx")
    nm.add_all_qubit_quantum_error(noise.amplitude_damping_error(0.2), "ry")
    qc = to_circuit(5, [("ry", (3,), (0.3,)), ("cx", (0, 3), ()), ("ry", (0,), (0.5,)), ("cx", (3, 1), ())])
    rows, n_events, _ = noise.trajectory_program(qc, nm)
    counts, sched = _plan(5, rows, 1)
    bare = rows[(rows["flags"] & 0xFF) != _lib.OP_KRAUS2]
    c0, s0 = _plan(5, bare, 0)
    keep = sched[~_is_group(sched)]
    assert len(keep) == len(s0)
    for f in ("nq", "q0", "q1", "m"):
        assert np.array_equal(keep[f], s0[f]), f
    g = sched[_is_group(sched)]
    assert len(g) == 32 and np.all(g["flags"] & PRODUCT)
    assert np.all(g["q0"][:16] == 0) and np.all(g["q1"][:16] == 1)  # qubit 3 was routed next to qubit 0


# ---- malformed groups -----------------------------------------------------------------------------------
def _malformed_programs():
    """The cases of test_noise2_host._malformed_programs: the program of ops(3, 1) under model (b), whose
    groups hold 2 rows (and under (a), 16), broken one way each."""
    _, rows, _ = t2ref.program(3, 1, "b")
    g = int(np.flatnonzero((rows["flags"] & 0xFFFF) == _lib.OP_KRAUS2)[0])  # a group's first row
    assert int(rows["flags"][g]) == 3 | (2 << 16) and int(rows["flags"][g + 1]) == 3 | (1 << 8) | (2 << 16)
    dep = t2ref.program(3, 1, "a")[1]
    d = int(np.flatnonzero((dep["flags"] & 0xFFFF) == _lib.OP_KRAUS2)[0])
    out = []

    def case(label, base, edit):
        out.append((label, np.ascontiguousarray(edit(base.copy()))))

    def swap(r):
        r[[d + 1, d + 2]] = r[[d + 2, d + 1]]
        return r

    def setf(field, i, value):
        def edit(r):
            r[field][i] = value
            return r
        return edit

    def setm(i, e, value):
        def edit(r):
            r["m"][i, e] = value
            return r
        return edit

    def seventeen(r):
        r = np.concatenate([r[:d], np.repeat(r[d: d + 1], 17), r[d + 16:]])
        r["flags"][d: d + 17] = 3 | (np.arange(17) << 8) | (17 << 16)
        r["m"][d: d + 17] *= np.sqrt(16 / 17)
        return r

    case("k out of order", dep, swap)
    case("a group without its first row", rows, lambda r: np.delete(r, g))
    case("a group cut short by a gate", rows, lambda r: np.delete(r, g + 1))
    case("a group cut short by the program's end", dep, lambda r: r[: d + 9])
    case("k repeated", rows, setf("flags", g + 1, 3 | (2 << 16)))
    case("nk = 0", rows, lambda r: setf("flags", g + 1, 3 | (1 << 8))(setf("flags", g, 3)(r)))
    case("nk = 17", dep, seventeen)
    case("nk differs inside the group", rows, setf("flags", g + 1, 3 | (1 << 8) | (3 << 16)))
    case("qubits differ inside the group", rows, lambda r: setf("q1", g + 1, int(r["q0"][g]))(
        setf("q0", g + 1, int(r["q1"][g]))(r)))
    case("q0 = q1", rows, lambda r: setf("q1", g + 1, int(r["q0"][g]))(setf("q1", g, int(r["q0"][g]))(r)))
    case("a qubit out of range", rows, lambda r: setf("q1", g + 1, 3)(setf("q1", g, 3)(r)))
    case("a negative qubit", rows, lambda r: setf("q0", g + 1, -1)(setf("q0", g, -1)(r)))
    case("nq = 1", rows, setf("nq", g, 1))
    case("bits above nk", rows, setf("flags", g, 3 | (2 << 16) | (1 << 24)))
    case("a NaN entry", rows, setm(g + 1, 5, np.nan))
    case("an infinite entry", rows, setm(g, 0, np.inf))
    case("sum K^dag K off the identity", rows, setm(g, 0, 1.0 + 1e-8))
    return out


MALFORMED = _malformed_programs()


@pytest.mark.parametrize("label,rows", MALFORMED, ids=[label for label, _ in MALFORMED])
def test_malformed_groups_still_answer_err_arg(mode, label, rows):
    """Under mode 1 the five entry points check a group before any device call: AQC_ERR_ARG, no GPU."""
    lib = _lib.load()
    assert mode(1) == 0
    counts = np.zeros(7, dtype=np.int32)
    assert lib.aqc_mps_traj_plan(3, _lib.ptr(rows), len(rows), _lib.ptr(counts), None, 0) == -1, label
    assert lib.aqc_mps_traj_tomo_plan(3, _lib.ptr(rows), len(rows), _lib.ptr(counts), None, 0) == -1, label
    out = np.zeros((4, 1), dtype=np.uint64)
    rc = lib.aqc_mps_traj_sample(3, 8, 1e-16, 0, _lib.ptr(rows), len(rows), 4, ctypes.c_uint64(1), ctypes.c_uint64(0),
                                 None, _lib.ptr(out), None)
    assert rc == -1, label
    pairs = np.array([0, 1], dtype=np.int32)
    eff = np.ascontiguousarray(noise.readout_effects(3, None))
    tables = np.zeros((1, 9, 4), dtype=np.int64)
    rc = lib.aqc_mps_traj_pair_tomo(3, 8, 1e-16, 0, _lib.ptr(rows), len(rows), _lib.ptr(pairs), 1, _lib.ptr(eff), 4,
                                    ctypes.c_uint64(1), ctypes.c_uint64(0), None, _lib.ptr(tables), None)
    assert rc == -1, label
    codes = np.array([[3, 0, 1]], dtype=np.uint8)
    plus = np.zeros(1, dtype=np.int64)
    rc = lib.aqc_mps_traj_pauli_counts(3, 8, 1e-16, 0, _lib.ptr(rows), len(rows), _lib.ptr(codes), 1, _lib.ptr(eff), 4,
                                       ctypes.c_uint64(1), ctypes.c_uint64(0), None, _lib.ptr(plus), None, None, None)
    assert rc == -1, label
    # the well-formed program still plans
    good = np.ascontiguousarray(t2ref.program(3, 1, "b")[1])
    assert lib.aqc_mps_traj_plan(3, _lib.ptr(good), len(good), _lib.ptr(counts), None, 0) == 0


# ---- the restatement -----------------------------------------------------------------------------------
def test_restatement_agrees_with_its_parts():
    """mps_trajectory2_ref on a program without groups is mps_trajectory_ref, and its event loop is
    trajectory2_ref.evolve's under the wider band."""
    import mps_trajectory2_ref as m2ref
    import mps_trajectory_ref as mref
    from adaptaqc_amd.noise import trajectory_program
    from conftest import to_circuit

    nm = noise.NoiseModel()
    nm.add_all_qubit_quantum_error(noise.thermal_relaxation_error(50e3, 70e3, 5000), ["rx", "ry", "rz"])
    rows, n_events, _ = trajectory_program(to_circuit(4, ref.brickwork(4, 2, 9)), nm)
    u = ref.uniforms(3, 0, 20, n_events + 4)
    for got, want in zip(m2ref.trajectories(4, rows, u), mref.trajectories(4, rows, u)):
        assert np.array_equal(got, want)
    _, rows, n_events = t2ref.program(4, 3, "c")
    u = ref.uniforms(4, 0, 20, n_events + 4)
    psi, k, near, e = m2ref.evolve(4, rows, u)
    psi0, k0, near0, e0 = t2ref.evolve(4, rows, u)
    assert e == e0 == n_events and np.array_equal(k, k0) and np.array_equal(psi, psi0) and not (near0 & ~near).any()


# ---- the schedule replayed on Vidal tensors: the centre condition at every general group ----------------
def _dense(gam, lam):
    """The MPS contracted in site order: psi[s_0, ..., s_{n-1}]."""
    t = np.ones((1, 1), dtype=complex)
    for j, g in enumerate(gam):
        t = np.tensordot(t, lam[j][None, :, None] * g, axes=([-1], [1]))
    return t[0, ..., 0]


def _vidal_replay(n, sched, u):
    """One shot of a plan without the measurement sweep on Vidal tensors (theta, numpy.linalg.svd, lambda
    division; sigma^2 <= 1e-16 chopped), every event's weights from the LOCAL formula the device uses:
    the one-site rho of a Kraus row, rho = theta theta^dag of a general group, the constants of a
    product-unitary one.  Returns (psi in site order, choices, the largest deviation of a local rho from
    the contracted state's reduced density matrix)."""
    gam = [np.zeros((2, 1, 1), dtype=complex) for _ in range(n)]
    for g in gam:
        g[0, 0, 0] = 1.0
    lam = [np.ones(1) for _ in range(n + 1)]
    choices = []
    dev = 0.0

    def theta_of(p, g4):
        a = lam[p][None, :, None] * gam[p] * lam[p + 1][None, None, :]
        b = gam[p + 1] * lam[p + 2][None, None, :]
        return np.einsum("abst,slm,tmr->albr", g4, a, b)

    def split(theta, p):
        cl, cr = theta.shape[1], theta.shape[3]
        uu, s, vh = np.linalg.svd(theta.reshape(2 * cl, 2 * cr), full_matrices=False)
        keep = max(1, int(np.count_nonzero(s ** 2 > 1e-16)))
        uu, s, vh = uu[:, :keep], s[:keep], vh[:keep]
        lam[p + 1] = s / np.linalg.norm(s)
        gam[p] = uu.reshape(2, cl, keep) / lam[p][None, :, None]
        gam[p + 1] = vh.reshape(keep, 2, cr).transpose(1, 0, 2) / lam[p + 2][None, None, :]

    def rdm(sites):
        psi = _dense(gam, lam)
        m = np.moveaxis(psi, sites, range(len(sites))).reshape(2 ** len(sites), -1)
        return m @ m.conj().T

    i = 0
    while i < len(sched):
        row = sched[i]
        p, q1, flags, nq = int(row["q0"]), int(row["q1"]), int(row["flags"]), int(row["nq"])
        m = np.asarray(row["m"]).view(np.complex128)
        if flags == 0 and nq == 2:
            split(theta_of(p, m.reshape(2, 2, 2, 2)), p)
            i += 1
        elif flags == 0:
            gam[p] = np.einsum("st,tlr->slr", m[:4].reshape(2, 2), gam[p])
            i += 1
        elif flags & 0xFF == _lib.OP_KRAUS1:
            ks = [m[4 * k: 4 * k + 4].reshape(2, 2) for k in range(q1)]
            w = (lam[p] ** 2)[:, None] * (lam[p + 1] ** 2)[None, :]
            rho = np.einsum("lr,slr,tlr->st", w, gam[p], gam[p].conj())
            dev = max(dev, float(np.max(np.abs(rho - rdm([p])))))
            pk = np.array([max(0.0, float(np.real(np.trace(k.conj().T @ k @ rho)))) for k in ks])
            k = _choose(pk, u[len(choices)])
            choices.append(k)
            gam[p] = np.einsum("st,tlr->slr", ks[k] / np.sqrt(pk[k]), gam[p])
            i += 1
        else:
            nk = (flags >> 16) & 0xFF
            ks = [np.asarray(g["m"]).view(np.complex128).reshape(4, 4) for g in sched[i: i + nk]]
            if flags & PRODUCT:
                pk = np.array([float(np.real(np.trace(k.conj().T @ k))) / 4 for k in ks])
                k = _choose(pk, u[len(choices)])
                k4 = (ks[k] / np.sqrt(pk[k])).reshape(2, 2, 2, 2)  # [s_p', s_q1', s_p, s_q1] = A (x) B
                at = np.unravel_index(np.argmax(np.abs(k4)), k4.shape)
                gam[p] = np.einsum("st,tlr->slr", k4[:, at[1], :, at[3]] / k4[at], gam[p])
                gam[q1] = np.einsum("st,tlr->slr", k4[at[0], :, at[2], :], gam[q1])
            else:
                theta = theta_of(p, np.eye(4).reshape(2, 2, 2, 2))
                t4 = theta.transpose(0, 2, 1, 3).reshape(4, -1)  # [2 s1 + s2][l, r]
                rho = t4 @ t4.conj().T
                dev = max(dev, float(np.max(np.abs(rho - rdm([p, p + 1])))))
                pk = np.array([max(0.0, float(np.real(np.trace(k.conj().T @ k @ rho)))) for k in ks])
                k = _choose(pk, u[len(choices)])
                split(np.einsum("abst,sltr->albr", (ks[k] / np.sqrt(pk[k])).reshape(2, 2, 2, 2), theta), p)
            choices.append(k)
            i += nk
    return _dense(gam, lam), np.array(choices, dtype=np.uint8), dev


VIDAL = [(3, 1, "c"), (3, 1, "a"), (4, 3, "c"), (4, 3, "b"), (5, 2, "c"), (6, 2, "a")]


@pytest.mark.parametrize("n,depth,which", VIDAL)
@pytest.mark.parametrize("correlated", [1, 2])
def test_schedule_replayed_on_vidal_tensors(n, depth, which, correlated):
    """At every Kraus row and every general group the local rho the device forms equals the contracted
    state's reduced density matrix to 1e-10 -- the a / b bookkeeping behind a general group, whose
    operator is not unitary -- and states and choices equal the dense restatement's."""
    _, rows, n_events = t2ref.program(n, depth, which)
    _, sched = _plan(n, rows, correlated, measure=False)
    shots = 6
    u = ref.uniforms(5 + n, 0, shots, n_events)
    want_psi, want_k, near, _ = t2ref.evolve(n, rows, u)
    assert not near.any()
    worst = off = 0.0
    for s in range(shots):
        psi, choices, dev = _vidal_replay(n, sched, u[s])
        assert np.array_equal(choices, want_k[s]), s
        worst = max(worst, dev)
        off = max(off, float(np.max(np.abs(psi.transpose(*range(n - 1, -1, -1)).reshape(-1) - want_psi[s]))))
    print(f"n={n} model {which} mode {correlated}: local rho off by at most {worst:.2e}, states by {off:.2e}")
    assert worst < 1e-10 and off < 1e-8  # (the chop at sigma^2 <= 1e-16 moves amplitudes by up to 1e-8)
