"""The pair-transition reader and the route it opens, on the device: aqc_dm_pair_transitions against numpy at
every size where its waves and workgroups are filled differently, against the one-qubit transition reader and
the pair environments, ``general_gradients`` with an entangling starting circuit and for the local cost against
parameter shifts of whole programs on ``DeviceDM.run``, ``candidate_layer_costs`` against the backend's costs,
and a compile with ``method="general_gradient"`` from an entangling starting circuit.

Tolerances: 1e-10, the density-matrix readers' parity tolerance (tests/test_gpu_dm.py), for the reader on inputs
of Frobenius norm 1 and for costs from one reader call; 1e-9 where a gradient or a cost goes through whole
evolutions (tests/test_gpu_dm_gradient.py)."""
import functools
from types import SimpleNamespace

import numpy as np
import pytest

import dm_gradient_ref as gref
import dm_pair_transition_ref as pref
import dm_ref as dref
import dm_sweep_ref as sref
import trajectory2_ref as t2ref
from conftest import to_circuit

pytestmark = pytest.mark.gpu

TOL = 1e-10


def _dm(n, x=None):
    from adaptaqc_amd.device import DeviceDM

    dev = DeviceDM(n)
    if x is not None:
        dev.set(x)
    return dev


def _split_n():
    """The smallest n at which a pair is spread over more than one workgroup (no GPU call)."""
    from adaptaqc_amd.device import dm_pair_transitions_split

    return min(n for n in range(2, 14) if dm_pair_transitions_split(n, len(_pairs(n))) >= 2)


def _pairs(n):
    """(0, 1), (0, n-1), (n-2, n-1), a reversed pair and the interior pairs of tests/test_gpu_dm_gradient.py."""
    pairs = [(0, 1), (0, n - 1), (n - 2, n - 1), (n - 1, 0)]
    if n >= 5:
        pairs += [(1, n - 2), (n - 3, 1)]
    return list(dict.fromkeys(pairs))


def _unit(x):
    return x / np.linalg.norm(x)


# ---- the reader against numpy -------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _numpy_transitions(n):
    """(a, b, the transition matrices of _pairs(n) in numpy): two different non-Hermitian matrices of norm 1."""
    a, b = _unit(sref.random_matrix(n, 1500 + n)), _unit(sref.random_matrix(n, 1600 + n))
    want = np.stack([pref.pair_transition(a, b, n, p, q) for p, q in _pairs(n)])
    for x in (a, b, want):
        x.setflags(write=False)
    return a, b, want


# n = 2: K = 4^(n-2) = 1, one lane group of one wave; 3: K = 4, one MFMA step of one wave; 4: K = 16, one step a
# wave; 5: K = 64, one unrolled iteration a wave; 6: K = 256, four; and the first n with more than one workgroup
@pytest.mark.parametrize("n", [2, 3, 4, 5, 6, "split"])
def test_pair_transitions_against_numpy(n):
    from adaptaqc_amd.device import dm_pair_transitions_split

    n = _split_n() if n == "split" else n
    a, b, want = _numpy_transitions(n)
    da, db = _dm(n, a), _dm(n, b)
    got = da.pair_transitions(db, _pairs(n))
    err = np.max(np.abs(got - want))
    split = dm_pair_transitions_split(n, len(_pairs(n)))
    print(f"n={n}: {len(want)} pairs over {split} workgroup(s) each, max entry error {err:.3e} "
          f"(largest entry {np.max(np.abs(want)):.3e})")
    assert n <= 9 and got.shape == (len(_pairs(n)), 16, 16)
    assert err <= TOL
    assert np.array_equal(da.pair_transitions(db, _pairs(n)), got)  # two calls, the same bits
    assert np.array_equal(da.pair_transitions(db, [_pairs(n)[-1]])[0], got[-1])  # whatever the launch's pairs
    # the other way round is the adjoint: T_ba[j', j] = conj(T_ab[j, j'])
    assert np.max(np.abs(db.pair_transitions(da, _pairs(n)) - got.conj().transpose(0, 2, 1))) <= TOL
    # a == b
    same = np.stack([pref.pair_transition(a, a, n, p, q) for p, q in _pairs(n)])
    assert np.max(np.abs(da.pair_transitions(da, _pairs(n)) - same)) <= TOL
    assert np.array_equal(da.get(), a) and np.array_equal(db.get(), b)  # a reader


def test_pair_transitions_argument_errors():
    from adaptaqc_amd._lib import AqcError

    dev, other = _dm(3), _dm(4)
    for bad in [(0, 3), (-1, 1), (2, 2)]:
        with pytest.raises(AqcError, match="aqc_dm_pair_transitions"):
            dev.pair_transitions(dev, [(0, 1), bad])
    with pytest.raises(AqcError, match="aqc_dm_pair_transitions"):
        dev.pair_transitions(other, [(0, 1)])
    one = _dm(1)
    with pytest.raises(AqcError, match="aqc_dm_pair_transitions"):
        one.pair_transitions(one, [(0, 1)])
    with pytest.raises(AqcError, match="aqc_dm_pair_transitions"):
        dev.pair_transitions(dev, [(0, 1)] * 4097)
    assert dev.pair_transitions(dev, []).shape == (0, 16, 16)


# ---- against the readers that already exist -------------------------------------------------------------
N_C = 9  # 64 workgroups a pair


@functools.lru_cache(maxsize=None)
def _nine():
    rng = np.random.default_rng(1700)
    dim = 2 ** N_C
    return tuple(_unit(rng.standard_normal((dim, dim)) + 1j * rng.standard_normal((dim, dim))) for _ in range(2))


def test_contraction_is_the_one_qubit_transition():
    a, b = _nine()
    da, db = _dm(N_C, a), _dm(N_C, b)
    pairs = _pairs(N_C)
    got = da.pair_transitions(db, pairs)
    single = {q: da.transition(db, q) for q in sorted({q for p in pairs for q in p})}
    worst = 0.0
    for (p, q), t in zip(pairs, got):
        for which, qubit in (("lo", min(p, q)), ("hi", max(p, q))):
            worst = max(worst, float(np.max(np.abs(pref.contract(t, which) - single[qubit]))))
    print(f"n={N_C}: max entry error {worst:.3e}")
    assert worst <= TOL
    assert max(np.max(np.abs(t)) for t in single.values()) > 1e-3


def test_product_observable_gives_the_pair_environments():
    _, b = _nine()
    eff = gref.random_effects(N_C, 1800, "full")
    m = dref.kron_all([gref.unpack(e) for e in eff])
    dm, db = _dm(N_C, m), _dm(N_C, b)
    pairs = _pairs(N_C)
    got = dm.pair_transitions(db, pairs)
    envs = db.pair_envs(pairs, eff)
    worst = 0.0
    for (p, q), t, r in zip(pairs, got, envs):
        lo, hi = min(p, q), max(p, q)
        e_pair = np.kron(gref.unpack(eff[hi]), gref.unpack(eff[lo]))
        want = np.outer(e_pair.reshape(-1, order="F").conj(), r.reshape(-1, order="F"))
        worst = max(worst, float(np.max(np.abs(t - want))))
    print(f"n={N_C}: max entry error {worst:.3e} (largest environment entry {np.max(np.abs(envs)):.3e})")
    assert worst <= TOL


# ---- gradients -------------------------------------------------------------------------------------------
N_G = 4


def _noise():
    from adaptaqc_amd.utils.circuit_operations import create_noisemodel

    return create_noisemodel(50e-3, 70e-3, log_fidelities=False)


def _compiler(nm, start_ops, backend, n=N_G, **kw):
    from adaptaqc_amd.compilers import AdaptCompiler, AdaptConfig

    local = kw.pop("optimise_local_cost", False)
    return AdaptCompiler(to_circuit(n, gref.case(n, False)[0]), backend=backend,
                         adapt_config=AdaptConfig(method="general_gradient", **kw), execute_kwargs={"noise_model": nm},
                         starting_circuit=to_circuit(n, start_ops) if start_ops else None, optimise_local_cost=local)


@functools.lru_cache(maxsize=None)
def _cost_backend():
    """A backend of its own for the costs of whole programs: the tested one's caches stay as they are."""
    from adaptaqc_amd.backends import DensityMatrixBackend

    return DensityMatrixBackend()


def _whole_cost(circuit, nm, cost):
    """``evaluate_global_cost`` / ``evaluate_local_cost`` of ``circuit``: one evolution of the whole program."""
    fake = SimpleNamespace(full_circuit=circuit, execute_kwargs={"noise_model": nm})
    be = _cost_backend()
    return be.evaluate_global_cost(fake) if cost == "global" else be.evaluate_local_cost(fake)


def _shift_gradients(comp, nm, layer_ops, rotoselect, cost="global"):
    """Per pair of the compiler's coupling map, sqrt(sum g^2), g = [C(+pi/2) - C(-pi/2)] / 2 of the whole program
    with the candidate layer inserted at the end of the variational range: every rotation of the layer, under
    every name with ``rotoselect``, the other rotations at 0 (tests/dm_gradient_ref's rule)."""
    from adaptaqc_amd.utils import circuit_operations as co

    out = []
    end = comp.variational_circuit_range()[1]
    for c, t in comp.coupling_map:
        total = 0.0
        for i, (name, qs, _) in enumerate(layer_ops):
            if name not in gref.ROT:
                continue
            for op in (gref.ROT if rotoselect else (name,)):
                costs = []
                for theta in (np.pi / 2, -np.pi / 2):
                    cand = list(layer_ops)
                    cand[i] = (op, qs, (theta,))
                    qc = comp.full_circuit.copy()
                    co.add_to_circuit(qc, to_circuit(2, cand), end, qubit_subset=[c, t])
                    costs.append(_whole_cost(qc, nm, cost))
                total += ((costs[0] - costs[1]) / 2) ** 2
        out.append(np.sqrt(total))
    return np.array(out)


def _layer_ops(comp):
    return [(i.operation.name, tuple(i.qubits), tuple(i.operation.params)) for i in comp.layer_2q_gate.data]


@pytest.mark.parametrize("cost", ["global", "local"])
def test_gradients_behind_an_entangling_starting_circuit(cost):
    from adaptaqc_amd.backends import DensityMatrixBackend

    nm = _noise()
    be = DensityMatrixBackend(pair_transitions=True, gradient_cost=cost)
    comp = _compiler(nm, pref.entangling_start(N_G), be)
    assert not be._product_right_hand_side(comp)
    got = np.array(be.general_gradients(comp))
    want = _shift_gradients(comp, nm, _layer_ops(comp), True, cost)
    err = np.max(np.abs(got - want))
    print(f"{cost}: gradients {want}, max error {err:.3e}")
    assert len(got) == len(comp.coupling_map) == 6
    assert err <= 1e-9
    assert want.max() > 1e-3 and np.ptp(want) > 1e-4  # non-trivial, and the pairs are told apart
    assert be.backward_passes == 1
    assert np.array_equal(np.array(be.general_gradients(comp)), got) and be.backward_passes == 1  # M is kept
    # gradient_cost="compiler" follows the compiler's flag
    follow = DensityMatrixBackend(pair_transitions=True, gradient_cost="compiler")
    comp2 = _compiler(nm, pref.entangling_start(N_G), follow, optimise_local_cost=(cost == "local"))
    assert np.max(np.abs(np.array(follow.general_gradients(comp2)) - got)) <= TOL


def test_both_routes_agree_on_a_product_start():
    from adaptaqc_amd.backends import DensityMatrixBackend

    nm = _noise()
    start_ops = gref.case(N_G, True)[2]
    default = _compiler(nm, start_ops, DensityMatrixBackend())
    want = np.array(default.backend.general_gradients(default))
    always = DensityMatrixBackend(pair_transitions="always")
    got = np.array(always.general_gradients(_compiler(nm, start_ops, always)))
    opt = DensityMatrixBackend(pair_transitions=True)
    same = np.array(opt.general_gradients(_compiler(nm, start_ops, opt)))
    err = np.max(np.abs(got - want))
    print(f"gradients {want}, max gap between the routes {err:.3e}")
    assert err <= TOL
    assert want.max() > 1e-3
    assert always.backward_passes == 1
    assert np.array_equal(same, want) and opt.backward_passes == 0  # True: the cheaper route where it applies


def test_candidate_layer_costs():
    from adaptaqc_amd.backends import DensityMatrixBackend
    from adaptaqc_amd.utils import circuit_operations as co

    nm = _noise()
    be = DensityMatrixBackend(pair_transitions=True)
    comp = _compiler(nm, pref.entangling_start(N_G), be)
    rng = np.random.default_rng(1900)
    layers = []
    for k in range(5):
        shape = gref.MIXED if k % 2 else gref.THIN
        ops = [(name, qs, (float(rng.uniform(-np.pi, np.pi)),) if name in gref.ROT else ()) for name, qs, _ in shape]
        layers.append(to_circuit(2, ops))
    pair = (2, 0)
    end = comp.variational_circuit_range()[1]
    for cost in ("global", "local"):
        got = np.array(be.candidate_layer_costs(comp, pair, layers, cost))
        want = []
        for layer in layers:
            qc = comp.full_circuit.copy()
            co.add_to_circuit(qc, layer, end, qubit_subset=list(pair))
            want.append(_whole_cost(qc, nm, cost))
        err = np.max(np.abs(got - np.array(want)))
        print(f"{cost}: costs {np.array(want)}, max error {err:.3e}")
        assert err <= TOL
        assert np.ptp(want) > 1e-3  # the layers are told apart
    # no layer at all is the backend's own cost
    empty = to_circuit(2, [])
    assert abs(be.candidate_layer_costs(comp, pair, [empty])[0] - _whole_cost(comp.full_circuit, nm, "global")) <= TOL
    assert be.backward_passes == 2  # one per cost


# ---- a compile -------------------------------------------------------------------------------------------
def test_compile_from_an_entangling_starting_circuit():
    from adaptaqc_amd.backends import DensityMatrixBackend
    from adaptaqc_amd.noise import trajectory_program

    nm = _noise()
    be = DensityMatrixBackend(pair_transitions=True)
    comp = _compiler(nm, pref.entangling_start(N_G), be, max_layers=3)
    seen = []  # the circuit in front of every pair selection
    inner = comp._get_all_qubit_pair_gradients

    def spy():
        seen.append(comp.full_circuit.copy())
        return inner()

    comp._get_all_qubit_pair_gradients = spy
    result = comp.compile()
    layers = len(result.qubit_pair_history)
    assert layers >= 2 and result.method_history == ["general_gradient"] * layers
    assert len(comp.general_gradient_history) == layers == len(seen)
    layer_ops = _layer_ops(comp)
    final = comp.full_circuit
    for k, qc in enumerate(seen):
        comp.full_circuit = qc
        want = _shift_gradients(comp, nm, layer_ops, True)
        got = np.array(comp.general_gradient_history[k])
        err = np.max(np.abs(got - want))
        print(f"layer {k}: pair {result.qubit_pair_history[k]}, gradients {got}, max error {err:.3e}")
        assert err <= 1e-9
    comp.full_circuit = final
    rows, _, _ = trajectory_program(gref.with_measures(final), nm)
    rho = t2ref.density_matrix(N_G, rows)
    print(f"cost history {result.global_cost_history}")
    assert abs(result.global_cost_history[-1] - (1 - rho[0, 0].real / np.trace(rho).real)) <= 1e-9
    assert be.backward_passes == 1  # the right-hand side never changes: M is pulled back once a compile
    refused = _compiler(nm, pref.entangling_start(N_G), DensityMatrixBackend(), max_layers=3)
    with pytest.raises(NotImplementedError, match="starting_circuit"):
        refused.compile()
