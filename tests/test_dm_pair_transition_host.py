"""The host side of the pair-transition route of the noise-aware general gradient: the numpy restatement of
aqc_dm_pair_transitions against the identities that tie it to the one-qubit transition matrix and to the pair
environments, gradients.noisy_grads_from_transitions on numpy-built matrices against the environments route,
against numpy evolutions of every shifted circuit with an entangling right-hand side and for the local cost,
aqc_dm_pair_transitions_plan, and DensityMatrixBackend's options.  No GPU."""
import ctypes
import functools

import numpy as np
import pytest

import dm_gradient_ref as gref
import dm_pair_transition_ref as pref
import dm_ref as dref
import dm_sweep_ref as sref
import trajectory2_ref as t2ref
from adaptaqc_amd.noise import trajectory_program
from conftest import to_circuit


def _pairs(n):
    """tests/test_gpu_dm_gradient.py's pairs: the corners, a reversed pair and the interior ones."""
    pairs = [(0, 1), (0, n - 1), (n - 2, n - 1), (n - 1, 0)]
    if n >= 5:
        pairs += [(1, n - 2), (n - 3, 1)]
    return list(dict.fromkeys(pairs))


# ---- the restatement against the identities ------------------------------------------------------------
@pytest.mark.parametrize("n", [4, 5])
def test_reference_contracts_to_the_one_qubit_transition(n):
    a, b = sref.random_matrix(n, 1100 + n), sref.random_matrix(n, 1200 + n)
    assert any(p > q for p, q in _pairs(n))
    worst = 0.0
    for p, q in _pairs(n):
        t = pref.pair_transition(a, b, n, p, q)
        assert t.shape == (16, 16)
        for which, qubit in (("lo", min(p, q)), ("hi", max(p, q))):
            worst = max(worst, float(np.max(np.abs(pref.contract(t, which) - sref.transition(a, b, n, qubit)))))
        assert np.array_equal(t, pref.pair_transition(a, b, n, q, p))  # lo / hi, whatever the order listed
    print(f"n={n}: max entry error {worst:.3e}")
    assert worst <= 1e-12


@pytest.mark.parametrize("n", [4, 5])
def test_reference_of_a_product_observable_is_the_pair_environment(n):
    """M = (x) E_q: T = conj(vec E_pair) (x) vec R, R the pair's environment."""
    rho = sref.random_matrix(n, 1300 + n)
    eff = gref.random_effects(n, 1400 + n, "full")
    m = dref.kron_all([gref.unpack(e) for e in eff])
    worst = 0.0
    for p, q in _pairs(n):
        lo, hi = min(p, q), max(p, q)
        e_pair = np.kron(gref.unpack(eff[hi]), gref.unpack(eff[lo]))
        r = gref.pair_env(rho, n, p, q, eff)
        want = np.outer(e_pair.reshape(-1, order="F").conj(), r.reshape(-1, order="F"))
        worst = max(worst, float(np.max(np.abs(pref.pair_transition(m, rho, n, p, q) - want))))
    print(f"n={n}: max entry error {worst:.3e}")
    assert worst <= 1e-12


# ---- noisy_grads_from_transitions ----------------------------------------------------------------------
def _model(noisy):
    return gref.model() if noisy else None


@functools.lru_cache(maxsize=None)
def _rho(n, noisy):
    """rho in front of the layer: dm_gradient_ref.case's brickwork under the model."""
    left = gref.case(n, False)[0]
    rho = t2ref.density_matrix(n, trajectory_program(to_circuit(n, left), _model(noisy))[0])
    rho.setflags(write=False)
    return rho


def _transitions(n, right, noisy, cost, cmap):
    m = pref.pulled_back(n, right, _model(noisy), cost)
    return np.stack([pref.pair_transition(m, _rho(n, noisy), n, c, t) for c, t in cmap])


@pytest.mark.parametrize("layer,rotoselect", [("THIN", True), ("MIXED", False)])
@pytest.mark.parametrize("noisy", [True, False])
@pytest.mark.parametrize("n", [3, 4])
def test_transition_gradients_equal_the_environment_gradients(n, noisy, layer, rotoselect):
    """A product right-hand side, the global cost: both routes apply."""
    from adaptaqc_amd import noise
    from adaptaqc_amd.utils.gradients import noisy_grads_from_envs, noisy_grads_from_transitions

    nm = _model(noisy)
    _, right, _ = gref.case(n, True)
    cmap = gref.full_cmap(n)
    rho = _rho(n, noisy)
    trace = np.trace(rho).real
    circ = to_circuit(2, getattr(gref, layer))
    rhs = gref.with_measures(to_circuit(n, right))
    effects = noise.terminal_effects(n, rhs.data, rhs, nm)
    envs = np.stack([gref.pair_env(rho, n, c, t, effects) for c, t in cmap])
    want = np.array(noisy_grads_from_envs(envs, trace, effects, circ, cmap, nm, rotoselect))
    trans = _transitions(n, right, noisy, "global", cmap)
    got = np.array(noisy_grads_from_transitions(trans, trace, circ, cmap, nm, rotoselect, -1.0))
    err = np.max(np.abs(got - want))
    print(f"n={n} noisy={noisy} {layer}: gradients {want}, max error {err:.3e}")
    assert err <= 1e-10
    assert want.max() > 0  # (not a comparison of zeros)
    # only the sign's square enters
    assert np.array_equal(got, noisy_grads_from_transitions(trans, trace, circ, cmap, nm, rotoselect, 1.0))


@pytest.mark.parametrize("layer,rotoselect", [("THIN", True), ("MIXED", False)])
@pytest.mark.parametrize("noisy", [True, False])
@pytest.mark.parametrize("cost", ["global", "local"])
def test_transition_gradients_against_brute_force_behind_an_entangling_right_hand_side(cost, noisy, layer, rotoselect):
    from adaptaqc_amd.utils.gradients import noisy_grads_from_transitions

    n = 3
    nm = _model(noisy)
    ops = getattr(gref, layer)
    left, right = gref.case(n, False)[0], pref.ENTANGLING_RIGHT[n]
    cmap = gref.full_cmap(n)
    trans = _transitions(n, right, noisy, cost, cmap)
    got = np.array(noisy_grads_from_transitions(trans, np.trace(_rho(n, noisy)).real, to_circuit(2, ops), cmap, nm,
                                                rotoselect, -1.0 if cost == "global" else 1.0))
    brute = gref.brute_force_gradients if cost == "global" else functools.partial(
        pref.brute_force_gradients, cost=pref.local_cost)
    want = np.array(brute(n, left, right, ops, cmap, nm, rotoselect))
    err = np.max(np.abs(got - want))
    print(f"{cost} noisy={noisy} {layer}: gradients {want}, max error {err:.3e}")
    assert err <= 1e-9
    assert want.max() > 0  # (not a comparison of zeros)


def test_the_brute_force_of_this_file_restates_dm_gradient_ref():
    n = 3
    left, right = gref.case(n, False)[0], pref.ENTANGLING_RIGHT[n]
    cmap = gref.full_cmap(n)[:2]
    a = gref.brute_force_gradients(n, left, right, gref.THIN, cmap, gref.model(), True)
    b = pref.brute_force_gradients(n, left, right, gref.THIN, cmap, gref.model(), True, pref.global_cost)
    assert np.array_equal(a, b)


def test_transition_gradient_argument_errors():
    from adaptaqc_amd.utils.gradients import noisy_grads_from_transitions

    cmap = gref.full_cmap(3)
    trans = np.zeros((len(cmap), 16, 16), dtype=complex)
    bad = to_circuit(2, [("rz", (0,), (0.0,)), ("cz", (0, 1), ())])
    with pytest.raises(ValueError, match="rx, ry, rz and cx"):
        noisy_grads_from_transitions(trans, 1.0, bad, cmap, None, True, -1.0)
    with pytest.raises(ValueError):
        noisy_grads_from_transitions(trans[:1], 1.0, to_circuit(2, gref.THIN), cmap, None, True, -1.0)


# ---- the plan and the exports --------------------------------------------------------------------------
def test_plan_of_the_reader():
    from adaptaqc_amd._lib import AqcError
    from adaptaqc_amd.device import dm_pair_transitions_split

    for n in range(2, 7):  # 4^(n-2) <= 256: one workgroup a pair
        assert dm_pair_transitions_split(n) == 1 and dm_pair_transitions_split(n, 66) == 1
    splits = {n: dm_pair_transitions_split(n, 6) for n in range(2, 14)}
    print(f"workgroups a pair, 6 pairs: {splits}")
    assert min(n for n, s in splits.items() if s >= 2) <= 9
    assert all(1 <= s <= 256 and s & (s - 1) == 0 for s in splits.values())
    assert all(splits[n] <= splits[n + 1] for n in range(2, 13))
    assert all(s <= 4 ** (n - 2) for n, s in splits.items())  # never more workgroups than values of o
    assert max(splits.values()) == 256
    for n in range(2, 14):  # many pairs: the partials stay bounded
        assert dm_pair_transitions_split(n, 4096) * 4096 <= 8192
    for n, npairs in [(1, 1), (14, 1), (0, 1), (5, 0), (5, -1), (5, 4097)]:
        with pytest.raises(AqcError, match="aqc_dm_pair_transitions_plan"):
            dm_pair_transitions_split(n, npairs)


def test_exports_and_signatures():
    from adaptaqc_amd import _lib

    for name, want in [("aqc_dm_pair_transitions", [ctypes.c_void_p] * 3 + [ctypes.c_int, ctypes.c_void_p]),
                       ("aqc_dm_pair_transitions_plan", [ctypes.c_int, ctypes.c_int, ctypes.POINTER(ctypes.c_int)])]:
        assert name in _lib.EXPORTS
        args, res = _lib._SIGS[name]
        assert list(args) == want and res is ctypes.c_int
        fn = getattr(_lib.load(), name)
        assert list(fn.argtypes) == want and fn.restype is ctypes.c_int


# ---- the backend's options -----------------------------------------------------------------------------
def _entangling_compiler(backend, n=3, **kw):
    from adaptaqc_amd.compilers import AdaptCompiler, AdaptConfig

    return AdaptCompiler(to_circuit(n, gref.case(n, False)[0]), backend=backend,
                         adapt_config=AdaptConfig(method="general_gradient"), execute_kwargs={"noise_model": gref.model()},
                         starting_circuit=to_circuit(n, pref.entangling_start(n)), **kw)


def test_backend_options():
    from adaptaqc_amd.backends import DensityMatrixBackend

    with pytest.raises(ValueError, match="pair_transitions") as info:
        DensityMatrixBackend(gradient_cost="local")
    assert "gradient_cost" in str(info.value)
    for kw in [{"pair_transitions": "sometimes"}, {"pair_transitions": 2}, {"gradient_cost": "soft"},
               {"pair_transitions": True, "gradient_cost": None}]:
        with pytest.raises(ValueError):
            DensityMatrixBackend(**kw)
    for mode in (True, "always"):
        for cost in ("global", "local", "compiler"):
            be = DensityMatrixBackend(pair_transitions=mode, gradient_cost=cost)
            assert (be.pair_transitions, be.gradient_cost, be.backward_passes) == (mode, cost, 0)
    be = DensityMatrixBackend()
    assert (be.pair_transitions, be.gradient_cost) == (False, "global")


def test_default_backend_still_refuses_an_entangling_start():
    from adaptaqc_amd.backends import DensityMatrixBackend

    comp = _entangling_compiler(DensityMatrixBackend())
    with pytest.raises(NotImplementedError, match="starting_circuit"):
        comp.backend.general_gradients(comp)


def test_compiler_cost_without_the_route_is_refused():
    """gradient_cost="compiler" on a compiler that optimises the local cost needs pair_transitions too."""
    from adaptaqc_amd.backends import DensityMatrixBackend

    comp = _entangling_compiler(DensityMatrixBackend(gradient_cost="compiler"), optimise_local_cost=True)
    with pytest.raises(ValueError, match="pair_transitions"):
        comp.backend.general_gradients(comp)


def test_the_cached_observable_is_not_pickled():
    import pickle

    from adaptaqc_amd.backends import DensityMatrixBackend

    be = DensityMatrixBackend(pair_transitions="always", gradient_cost="compiler")
    be._observables["global"] = (("key",), object())
    be.backward_passes = 3
    back = pickle.loads(pickle.dumps(be))
    assert (back.pair_transitions, back.gradient_cost) == ("always", "compiler")
    assert back._observables == {} and back.backward_passes == 0
