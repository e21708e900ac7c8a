"""Benchmark: overlap + gradient evaluations / s, 50-qubit MPS chi = 64 (BASELINE.json config 3).

One step, per rank, on a global batch of S = world * states_per_rank synthetic 50-qubit chi = 64
MPS (Vidal form, every bond at min(2^k, 2^(50-k), 64)), all resident in HBM.  The states are
random chi = 64 MPS with a product component near |0..0> (``near_product_mps``), so that the
gradients and overlaps are far from zero and every output of the step can be checked against the
oracle (on a plain random chi = 64 state every overlap with |0..0> is ~1e-8 and the gradients are
rounding noise).
  (i)  candidate sweep: gradient norm of the identity_resolvable layer (rotoselect generators,
       12 distinct, |s> = |0..0>) for all 1225 pairs of the full coupling map, pairs sharded
       across ranks by first qubit (each rank covers its shard for all S states), one RCCL
       all-gather of the float64 scores, and the per-state arg-max pair selection;
  (ii) overlap evaluations on this rank's own states_per_rank states: apply a thinly-dressed
       layer (4 rotations + CX) at pair distances 1, 2, 5, 25 (Aer swap routing, two-site SVD
       with max_chi = 64 truncation, sort back at save) and take 1 - |<0|psi>|^2.
value = (S * 1225 + S * 4) evaluations / step time (max over ranks): weak scaling.

A plain run sets up, warms up, times ``--steps`` steps and prints the result line (with the
per-family kernel times the library's timers collected during those steps, HIP events on the MPS
stream around every launch, and the dominant kernel's roofline worked out from them).
``--dump-outputs DIR`` also writes what the last timed step returned -- the gradient scores, the
per-state best pair and the overlap costs -- as ``DIR/<name>.npy`` (float64); the inputs are
seeded, so two builds can be compared output for output.

With ``--full`` also reported (outside the timed region):
  * each evaluation kind timed on its own (gradient / overlap evals per second) and the rate at
    the reference's own per-layer mix (1225 gradients + 113 Rotoselect overlap evaluations);
  * ``parity_check``: one state's 1225 gradients and arg-max pair and four overlap evaluations
    (one per distance, through the fused chain) against the oracle;
  * ``latency``: one state alone -- one overlap evaluation per distance, and one Rotoselect gate
    (``replace_with_best_1q_gate``'s 7 evaluations) on the cached-prefix path;
  * CPU baselines: the oracle's port of the reference algorithm (per-pair, per-generator MPS
    build + whole-psi dot; numpy LAPACK SVDs), one process per host core with single-threaded
    BLAS, on a bounded sample, run on rank 0 at N = 1 before the GPU is touched.
"""
import argparse
import json
import os
import sys
import time

os.environ.setdefault("OPENBLAS_NUM_THREADS", "1")  # CPU baseline workers: one core each
import numpy as np  # noqa: E402

ROOT = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, ROOT)

N_QUBITS = 50
CHI = 64
DISTANCES = (1, 2, 5, 25)
LAYER_A = 12
REF_OVERLAPS_PER_LAYER = 113  # Rotoselect evaluations per 4-rotation layer
FP64_PEAK_TFLOPS = 78.6  # MI355X dense FP64 (vector = matrix), MI355X_MICROARCH.md / SURVEY 8(d)
HBM_PEAK_GBS = 8000.0
# HBM traffic and executed FP64 work of k_chain per two-site update from the committed PMC passes
# of this round's code (tools/pmc_bench.sh, tools/pmc_exec.py); the previous round's as fallback
def _latest_profile(suffix):
    """The newest round's committed PMC result (profiles/rN_<suffix>, highest N)."""
    import re

    rounds = []
    for f in os.listdir(os.path.join(ROOT, "profiles")):
        m = re.fullmatch(r"r(\d+)_" + re.escape(suffix), f)
        if m:
            rounds.append(int(m.group(1)))
    return f"r{max(rounds)}_{suffix}" if rounds else f"r2_{suffix}"


TRAFFIC_JSON = _latest_profile("traffic.json")
EXEC_JSON = _latest_profile("exec_k_chain.json")


def vidal_from_tensors(A):
    """Vidal canonical form (Aer tuple) of the MPS with site tensors A[i] of shape (2, l, r):
    left-canonicalise by QR, then right-to-left SVDs give the lambdas; normalised."""
    A = [np.asarray(a, dtype=complex).copy() for a in A]
    n = len(A)
    for i in range(n - 1):  # left-canonicalise
        s, l, r = A[i].shape
        q, rr = np.linalg.qr(A[i].transpose(1, 0, 2).reshape(l * s, r))
        A[i] = q.reshape(l, s, -1).transpose(1, 0, 2)
        A[i + 1] = np.einsum("ab,sbc->sac", rr, A[i + 1])
    A[n - 1] /= np.linalg.norm(A[n - 1])
    lam = [None] * (n + 1)
    for i in range(n - 1, 0, -1):  # right sweep with SVDs -> lambdas
        s, l, r = A[i].shape
        u, sv, vh = np.linalg.svd(A[i].transpose(1, 0, 2).reshape(l, s * r), full_matrices=False)
        sv = sv / np.linalg.norm(sv)
        lam[i] = sv
        A[i] = vh.reshape(-1, s, r).transpose(1, 0, 2)
        A[i - 1] = np.einsum("sab,bc->sac", A[i - 1], u * sv[None, :])
    gam = []
    for i in range(n):
        g = A[i]
        if i == 0:
            g = g / lam[1][None, None, :]
        elif i < n - 1:
            g = g / lam[i + 1][None, None, :]
        gam.append((g[0].copy(), g[1].copy()))
    return gam, [lam[i] for i in range(1, n)]


def random_vidal_mps(n, chi, seed):
    """Random normalised MPS in exact Vidal canonical form (Aer tuple): bonds min(2^k, 2^(n-k), chi),
    complex-normal tensors."""
    rng = np.random.default_rng(seed)
    dims = [min(2 ** k, 2 ** (n - k), chi) for k in range(n + 1)]
    A = [(rng.standard_normal((2, dims[i], dims[i + 1])) + 1j * rng.standard_normal((2, dims[i], dims[i + 1])))
         for i in range(n)]
    return vidal_from_tensors(A)


def graded_vidal_mps(n, chi, seed, decay):
    """Random MPS whose Schmidt spectra decay geometrically: complex-normal tensors with right bond
    index k scaled by decay^k, canonicalised (Aer tuple; bonds min(2^k, 2^(n-k), chi)).  At decay
    0.9 and chi = 64 a thin layer's two-site spectra cross the reference example's truncation
    threshold 1e-8 (examples/advanced_mps_example.py:46) around the 50th value, so the tail rule of
    reduce_zeros decides the kept count (tests/test_gpu_threshold.py, tools/unbounded_profile.py)."""
    rng = np.random.default_rng(seed)
    dims = [min(2 ** k, 2 ** (n - k), chi) for k in range(n + 1)]
    A = []
    for i in range(n):
        t = rng.standard_normal((2, dims[i], dims[i + 1])) + 1j * rng.standard_normal((2, dims[i], dims[i + 1]))
        A.append(t * (decay ** np.arange(dims[i + 1]))[None, None, :])
    return vidal_from_tensors(A)


def near_product_mps(n, chi, seed, alpha=0.6):
    """|psi> ~ alpha |p> + |phi> in Vidal form: |p> a product of single-qubit states near |0>
    (angles 0.15-0.3, random phases), |phi> random with bonds min(2^k - 1, 2^(n-k) - 1, chi - 1),
    so that every bond of psi sits at min(2^k, 2^(n-k), chi) while the overlaps with |0..0>-like
    states (and so the gradients) are far from zero."""
    rng = np.random.default_rng(seed)
    dims = [1] + [min(2 ** k - 1, 2 ** (n - k) - 1, chi - 1) for k in range(1, n)] + [1]
    A = [(rng.standard_normal((2, dims[i], dims[i + 1])) + 1j * rng.standard_normal((2, dims[i], dims[i + 1])))
         for i in range(n)]
    gam, lam = vidal_from_tensors(A)
    phi = [np.stack(g) * (lam[i][None, None, :] if i < n - 1 else 1.0) for i, g in enumerate(gam)]
    out = []
    for i, t in enumerate(phi):  # block-diagonal sum with the near-|0> product chain
        s, l, r = t.shape
        li, ri = (1 if i == 0 else l + 1), (1 if i == n - 1 else r + 1)
        x = np.zeros((2, li, ri), dtype=complex)
        a, b = 0.15 * (1 + rng.random()), rng.uniform(-np.pi, np.pi)
        x[:, 0, 0] = (alpha if i == 0 else 1.0) * np.array([np.cos(a), np.exp(1j * b) * np.sin(a)])
        x[:, li - l:, ri - r:] = t
        out.append(x)
    return vidal_from_tensors(out)


def bench_states(n, chi, count, kind="near-product"):
    gen = near_product_mps if kind == "near-product" else random_vidal_mps
    return [gen(n, chi, 1000 + k) for k in range(count)]


THIN_AXES = ("rx", "rx", "rx", "rx")


def thin_layer_ops(a, b, angles, axes=THIN_AXES):
    """Thinly-dressed CNOT layer with rotoselect-style angles (and axes): r, r, cx, r, r."""
    from adaptaqc_amd import gates as G

    r = [G.one_qubit(axes[k], [angles[k]]) for k in range(4)]
    return [(r[0], (a,)), (r[1], (b,)), (G.TWO_QUBIT["cx"], (a, b)), (r[2], (a,)), (r[3], (b,))]


def thin_layer_oracle_ops(a, b, angles, axes=THIN_AXES):
    """The same layer as oracle ops (name, qubits, params)."""
    return [(axes[0], (a,), (float(angles[0]),)), (axes[1], (b,), (float(angles[1]),)), ("cx", (a, b), ()),
            (axes[2], (a,), (float(angles[2]),)), (axes[3], (b,), (float(angles[3]),))]


def layer_inputs():
    from adaptaqc_amd.utils import ansatzes
    from adaptaqc_amd.utils.gradients import get_generators_and_degeneracies, layer_operators

    layer = ansatzes.identity_resolvable()
    gens, deg = get_generators_and_degeneracies(layer, rotoselect=True, inverse=True)
    u0, gm = layer_operators(layer.inverse(), gens)
    return layer, gens, deg, u0, np.stack(gm)


def oracle_layer():
    """identity_resolvable (ansatzes.py:201-211) as oracle ops, its generators (rotoselect,
    inverse) and inverse."""
    from adaptaqc_amd.utils import ansatzes
    from oracle import gradients as ogr

    o_layer = [(i.operation.name, tuple(i.qubits), tuple(i.operation.params))
               for i in ansatzes.identity_resolvable().data]
    og, od = ogr.get_generators_and_degeneracies(o_layer, True, True)
    return o_layer, og, od, ogr.inverse_ops(o_layer)


def svd_nominal_flops(m, n):
    """LAPACK-style complex SVD with both singular-vector sets: 4 x (4m^2n + 8mn^2 + 9n^3), m >= n."""
    m, n = max(m, n), min(m, n)
    return 4.0 * (4 * m * m * n + 8 * m * n * n + 9 * n ** 3)


# ---------------------------------------------------------------------------------------------
# CPU baseline (oracle port of the reference structure), one process per core
# ---------------------------------------------------------------------------------------------
def _cpu_worker(args):
    from threadpoolctl import threadpool_limits

    with threadpool_limits(limits=1):  # one core per worker, whatever OMP/OPENBLAS_NUM_THREADS say
        return _cpu_worker_body(*args)


def _cpu_worker_body(kind, wid, budget_s, layer_seed):
    from oracle import adapt_host, gradients as ogr, mps as M

    q = near_product_mps(N_QUBITS, CHI, layer_seed)
    st = M.MPS.from_aer(q)
    n = N_QUBITS
    t0 = time.perf_counter()
    count = 0
    per_d = {}
    if kind == "overlap":
        rng = np.random.default_rng(100 + wid)
        k = wid
        while True:  # one evaluation per distance, round-robin from this worker's offset
            d = DISTANCES[k % len(DISTANCES)]
            ops = thin_layer_oracle_ops(LAYER_A, LAYER_A + d, rng.uniform(-np.pi, np.pi, 4))
            t1 = time.perf_counter()
            out = M.run_circuit(n, ops, 1e-16, CHI, mps=st)  # replay on the cached MPS + save
            _ = 1 - abs(M.mps_dot(out.preprocessed(), M.zero_mps(n))) ** 2
            per_d.setdefault(d, []).append(time.perf_counter() - t1)
            count += 1
            k += 1
            if time.perf_counter() - t0 > budget_s and count >= len(DISTANCES):
                break
    elif kind == "gradient_env":
        # like for like with the GPU's algorithm: whole environment-form sweeps (oracle/gradients.py,
        # the same factorisation through T_ab as the device sweep), pairs counted
        psi = st.preprocessed()
        _, og, od, inv0 = oracle_layer()
        cmap = adapt_host.coupling_map_full(n)
        while time.perf_counter() - t0 < budget_s or count == 0:
            t1 = time.perf_counter()
            ogr.general_grad_of_pairs_env(psi, n, inv0, og, od, cmap)
            per_d.setdefault("sweep", []).append(time.perf_counter() - t1)
            count += len(cmap)
    elif kind == "sweep_ref":
        # one whole reference-structure sweep split over the workers: worker wid computes pairs
        # wid, wid + W, ... once each (budget_s carries W); the workers' times add up to the 1-core
        # time of the sweep, every pair computed
        psi = st.preprocessed()
        _, og, od, inv0 = oracle_layer()
        cmap = adapt_host.coupling_map_full(n)
        mine = cmap[wid::int(budget_s)]
        ogr.general_grad_of_pairs_ref(psi, n, inv0, og, od, mine, (), 1e-16, CHI)
        count = len(mine)
    else:
        psi = st.preprocessed()
        _, og, od, inv0 = oracle_layer()
        cmap = adapt_host.coupling_map_full(n)
        order = np.random.default_rng(wid).permutation(len(cmap))
        while time.perf_counter() - t0 < budget_s or count == 0:
            pair = cmap[order[count % len(cmap)]]
            ogr.general_grad_of_pairs_ref(psi, n, inv0, og, od, [pair], (), 1e-16, CHI)
            count += 1
    return count, time.perf_counter() - t0, per_d


def host_description(workers):
    """The host the CPU baseline ran on: logical CPUs (os.cpu_count()), the CPUs this process may run
    on (sched_getaffinity), sockets and physical cores and the model name (/proc/cpuinfo), and why
    the baseline uses `workers` processes rather than every core."""
    model, phys, cores_per = None, set(), None
    try:
        with open("/proc/cpuinfo") as fh:
            for line in fh:
                k, _, v = line.partition(":")
                k, v = k.strip(), v.strip()
                if k == "model name" and model is None:
                    model = v
                elif k == "physical id":
                    phys.add(v)
                elif k == "cpu cores" and cores_per is None:
                    cores_per = int(v)
    except (OSError, ValueError):
        pass
    logical = os.cpu_count() or 1
    aff = len(os.sched_getaffinity(0)) if hasattr(os, "sched_getaffinity") else logical
    sockets = max(len(phys), 1)
    physical = sockets * cores_per if cores_per else logical
    return {"cpu_model": model, "host_logical_cpus": logical, "host_physical_cores": physical, "sockets": sockets,
            "affinity_cpus": aff, "workers": workers,
            "why_not_every_core": (f"the GPU box gives one GPU's process a share of {workers} CPUs of the node's "
                                   f"{logical} (os.cpu_count() reports the whole node; the pool asks jobs to size "
                                   "worker pools to that share), so the port runs on {workers} single-threaded "
                                   "processes; node_linear_bound scales it to every physical core, an upper bound "
                                   "(perfect scaling, no shared-memory-bandwidth loss)").replace("{workers}", str(workers))}


def cpu_baselines(budget_s, workers):
    """Gradient and overlap evaluations / s of the oracle port on `workers` processes (fork, before
    any GPU call), BLAS single-threaded in each.  Returns per-kind rates and the step-mix rate."""
    import multiprocessing as mp

    ctx = mp.get_context("fork")
    out = {}
    with ctx.Pool(workers) as pool:
        for kind in ("gradient", "gradient_env", "overlap", "sweep_ref"):
            b = float(workers) if kind == "sweep_ref" else budget_s
            res = pool.map(_cpu_worker, [(kind, w, b, 1000) for w in range(workers)])
            count = sum(c for c, _, _ in res)
            wall = max(t for _, t, _ in res)
            out[kind] = {"evals": count, "wall_s": wall, "evals_per_s": count / wall}
            if kind == "sweep_ref":  # every pair once: the workers' times add up to one core's sweep
                out[kind]["one_core_sweep_s"] = float(sum(t for _, t, _ in res))
            if kind == "gradient_env":
                out[kind]["one_core_sweep_s"] = float(np.median([x for _, _, pd in res for x in pd["sweep"]]))
            if kind == "overlap":  # one evaluation on one core, per distance (latency comparison)
                per_d = {}
                for _, _, pd in res:
                    for d, ts in pd.items():
                        per_d.setdefault(d, []).extend(ts)
                out[kind]["eval_ms_by_distance"] = {str(d): 1e3 * float(np.median(ts)) for d, ts in sorted(per_d.items())}
    return out


DUMP_MAX_BYTES = 16 << 20  # per dumped array (three arrays: well under 64 MB in all)


def dump_outputs(out_dir, rank, world, arrays):
    """Write what the last timed step returned as out_dir/<name>.npy (float64; device tensors are
    copied to the host).  With more than one rank every rank writes its own <name>_rank<r>.npy."""
    os.makedirs(out_dir, exist_ok=True)
    for name, a in arrays.items():
        if hasattr(a, "detach"):
            a = a.detach().cpu().numpy()
        a = np.ascontiguousarray(a, dtype=np.float64)
        if a.nbytes > DUMP_MAX_BYTES:  # a larger batch than the default: its leading rows
            a = a[: max(1, DUMP_MAX_BYTES // (a.nbytes // len(a)))]
        np.save(os.path.join(out_dir, name + (f"_rank{rank}" if world > 1 else "") + ".npy"), a)


# ---------------------------------------------------------------------------------------------
def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--gpus", type=int, default=1)
    ap.add_argument("--steps", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--states", type=int, default=256, help="states per rank")
    ap.add_argument("--distinct", type=int, default=8, help="distinct synthetic states generated")
    ap.add_argument("--state-kind", default="near-product", choices=("near-product", "random"))
    ap.add_argument("--dump-outputs", metavar="DIR", default=None,
                    help="write the last timed step's outputs (scores, best pairs, overlap costs) as DIR/<name>.npy")
    ap.add_argument("--full", action="store_true",
                    help="also the CPU baselines, each evaluation kind on its own, the parity check against the "
                         "oracle and the single-state latencies")
    ap.add_argument("--no-cpu-baseline", action="store_true", help="--full without the CPU baselines")
    ap.add_argument("--cpu-budget", type=float, default=4.0, help="seconds per CPU-baseline leg")
    ap.add_argument("--cpu-workers", type=int, default=0, help="0: min(16, OMP_NUM_THREADS or cores)")
    ap.add_argument("--cpu-settle", type=float, default=0.0, help="seconds of idle after the CPU-baseline leg")
    ap.add_argument("--no-parity", action="store_true", help="--full without the parity check")
    ap.add_argument("--no-latency", action="store_true", help="--full without the latency block")
    ap.add_argument("--no-pipeline", action="store_true",
                    help="sweep, then the overlap evaluations with a flag check after the chain (no overlap of host work)")
    ap.add_argument("--simulate-world", type=int, default=0,
                    help="projection only (1 process): rank 0's share of an N-GPU run -- pair shard of N, "
                         "sweep over N x states -- with the all-gather replaced by a local scatter")
    ap.add_argument("--shard", default="states", choices=("states", "pairs"),
                    help="states (default): each rank sweeps all 1225 pairs of its own states, one all-gather "
                         "of the per-state (best pair, score); pairs: every rank holds all N x states and "
                         "sweeps its pair shard, all-gather of the scores (the single-state layout)")
    ap.add_argument("--strong", action="store_true",
                    help="config 4 strong scaling: a fixed global batch of chi=128 sweeps sharded by state")
    ap.add_argument("--global-states", type=int, default=512, help="--strong: sweeps in the global batch")
    args = ap.parse_args()
    if args.steps < 1 or args.warmup < 0:
        ap.error("--steps must be at least 1 and --warmup at least 0")
    if args.strong:
        return strong_main(args)

    world = int(os.environ.get("WORLD_SIZE", "1"))
    rank = int(os.environ.get("RANK", "0"))
    local = int(os.environ.get("LOCAL_RANK", "0"))
    os.environ["AQC_DEVICE"] = str(local)

    cpu = None
    if args.full and rank == 0 and world == 1 and not args.no_cpu_baseline and not args.simulate_world:
        workers = args.cpu_workers or min(16, int(os.environ.get("OMP_NUM_THREADS", os.cpu_count() or 1)))
        cpu = cpu_baselines(args.cpu_budget, workers)
        cpu["workers"] = workers
        cpu["host"] = host_description(workers)
        if args.cpu_settle > 0:  # let the host's clocks recover before the GPU leg's host-side work
            time.sleep(args.cpu_settle)

    import torch
    import torch.distributed as dist

    torch.cuda.set_device(local)
    if world > 1:
        dist.init_process_group("nccl", device_id=torch.device("cuda", local))

    from adaptaqc_amd import _lib
    from adaptaqc_amd.device import (DeviceMPS, OpsBatch, apply_batch, copy_batch, overlap_zero_batch,
                                     pair_grads_batch)
    from adaptaqc_amd.sharding import PairShard, StateShard, best_pairs, gather_best, gather_scores
    from adaptaqc_amd.utils.constants import coupling_map_fully_entangled

    n, B = N_QUBITS, args.states
    sim = args.simulate_world if (args.simulate_world > 1 and world == 1) else 0
    shard_world = sim or world
    S = shard_world * B
    by_state = args.shard == "states"
    cmap = coupling_map_fully_entangled(n)
    # pair sharding: every rank sweeps its pairs over all S states; state sharding: all pairs of its
    # own B states (the shard below then covers every pair)
    shard = PairShard(cmap, n, 0 if by_state else rank, 1 if by_state else shard_world)
    sshard = StateShard(S, 0 if sim else rank, shard_world)
    layer, gens, deg, u0, gm = layer_inputs()
    svec = np.zeros((n, 2), complex)
    svec[:, 0] = 1.0

    distinct = bench_states(n, CHI, min(args.distinct, S), args.state_kind)
    states = []
    # state sharding holds only this rank's B states (global indices rank B ..); pair sharding all S
    for s in (range(rank * B, (rank + 1) * B) if by_state else range(S)):
        d = DeviceMPS(n, CHI, 1e-16, CHI)
        d.load_aer(distinct[s % len(distinct)])
        states.append(d)
    own = states if by_state else states[rank * B:(rank + 1) * B]
    work = [DeviceMPS(n, CHI, 1e-16, CHI) for _ in range(B * len(DISTANCES))]
    reload_src = [own[k // len(DISTANCES)] for k in range(len(work))]
    rng = np.random.default_rng(7)
    layer_angles, layer_ops = [], []
    for s in range(B):
        for d in DISTANCES:
            ang = rng.uniform(-np.pi, np.pi, 4)
            layer_angles.append(ang)
            layer_ops.append(_lib.ops_array(thin_layer_ops(LAYER_A, LAYER_A + d, ang)))
    # the op lists marshalled for the C ABI once (device.OpsBatch), as a caller re-evaluating the
    # same layer structure would (angles can change in place); the replay itself runs every step
    layer_batch = OpsBatch(layer_ops)
    prio = np.ones(len(cmap))
    local_scores = torch.zeros((len(states), max(len(shard.local_pairs), 1)), dtype=torch.float64, device="cuda")
    prio_t = torch.as_tensor(prio, device="cuda")

    def sweep_launch():
        # (i) the sharded candidate sweep's kernels (queued on the library stream)
        if by_state or shard.local_pairs:
            pair_grads_batch(states, svec, shard.local_pairs, u0, gm, deg, out=local_scores.data_ptr())

    def sweep_select():
        # ... then the all-gather + arg-max
        if by_state:
            # every pair of this rank's states, the per-state arg-max on the rank, then one all-gather
            # of (best pair, score) per state (RCCL over xGMI; the projection repeats rank 0's block)
            b, sc = best_pairs(local_scores, prio_t)
            if sim:
                return local_scores, b.repeat(sim)
            return local_scores, gather_best(b, sc, sshard)[0]
        if sim:  # projection: rank 0's scores scattered locally, no collective
            full = torch.zeros((S, len(cmap)), dtype=torch.float64, device="cuda")
            full[:, torch.as_tensor(shard.local_index, device="cuda")] = local_scores[:, : len(shard.local_pairs)]
        else:
            full = gather_scores(local_scores[:, : len(shard.local_pairs)], shard, nstates=S)
        return full, torch.argmax(full * prio_t, dim=1)

    def overlaps():
        # (ii) overlap evals on own states: reload the cached MPS, replay + save, <0|psi>
        copy_batch(work, reload_src)
        apply_batch(work, layer_batch, sort=True)
        return 1.0 - np.abs(overlap_zero_batch(work)) ** 2

    def sweep():
        sweep_launch()
        return sweep_select()

    def step():
        if args.no_pipeline:
            full, best = sweep()
            return full, best, overlaps()
        # the sweep's kernels first, then the chain's host preparation (~1-1.7 ms for 1024 states)
        # while the GPU runs them, then the arg-max / all-gather (queued behind the sweep, beside the
        # chain); the chain's flags are read after the cost read-back (one host wait per step).
        # (Preparing the chain after the arg-max left the GPU idle ~1.1 ms per step before the
        # chain in the traced timeline, tools/r4_bench_timeline.sh: 43.3 -> 42.6 ms per step.)
        sweep_launch()
        copy_batch(work, reload_src)
        apply_batch(work, layer_batch, sort=True, wait=False)
        full, best = sweep_select()
        # (the read-back of the overlaps also carries the chain's error flags: no check_batch)
        costs = 1.0 - np.abs(overlap_zero_batch(work)) ** 2
        return full, best, costs

    def barrier():
        torch.cuda.synchronize()
        if world > 1:
            dist.barrier()

    step_marks = []  # host clock after each timed step (each step ends on the cost read-back)

    def timed(fn, k):
        barrier()
        t0 = time.perf_counter()
        step_marks.clear()
        for _ in range(k):
            r = fn()
            step_marks.append(time.perf_counter() - t0)
        barrier()
        el = time.perf_counter() - t0
        if world > 1:
            t = torch.tensor([el], dtype=torch.float64, device="cuda")
            dist.all_reduce(t, op=dist.ReduceOp.MAX)
            el = float(t.item())
        return el, r

    # no Python garbage-collection pass inside the timed steps (measurement hygiene: a collection
    # holds the host while the GPU waits for the next launches).  On a quiet box it changes nothing
    # (profiles/r6_bench_gc_ab.json); two full lines run right after the whole GPU suite in the same
    # call showed 40.8-45.5 ms steps against 38.7-39.0 ms, with no cause pinned.  The collection
    # runs before the warm-up steps: between them and the timed ones it left the GPU idle long
    # enough that the first timed step ran ~1 ms slow.
    import gc

    gc.collect()
    if os.environ.get("AQC_BENCH_GC", "0") != "1":  # (AQC_BENCH_GC=1: collections on, for A/B)
        gc.disable()
    for _ in range(args.warmup):
        step()
    barrier()
    _lib.timing_reset()
    _lib.timing_enable(True)
    _lib.gram_stats()  # reset the Gram-path counters
    elapsed, (full, best, costs) = timed(step, args.steps)
    main_step_s = list(step_marks)
    gc.enable()
    _lib.timing_enable(False)
    gram = _lib.gram_stats()
    if world > 1:
        chk = best.to(torch.int64).clone()
        ref = chk.clone()
        dist.broadcast(ref, 0)
        assert torch.equal(chk, ref), "arg-max pair differs across ranks"
    ms_step = 1e3 * elapsed / args.steps
    evals_per_step = S * (len(cmap) + len(DISTANCES))
    value = evals_per_step * args.steps / elapsed

    fams = {f: _lib.timing_query(f)
            for f in ("mps_chain", "mps_svd", "mps_theta", "mps_split", "grad_chain", "mps_overlap0", "mps_copy")}

    if args.dump_outputs:
        dump_outputs(args.dump_outputs, rank, world,
                     {"pair_scores": full, "best_pair": best, "overlap_costs": costs})

    by_kind = None
    if args.full:
        # each evaluation kind on its own (outside the headline timed region)
        k_ph = max(2, args.steps // 2)
        t_sw, _ = timed(sweep, k_ph)
        t_ov, _ = timed(overlaps, k_ph)
        grad_rate = S * len(cmap) * k_ph / t_sw
        ov_rate = B * len(DISTANCES) * k_ph / t_ov * (shard_world if not sim else 1)
        mix_g, mix_o = len(cmap), REF_OVERLAPS_PER_LAYER
        ref_mix = (mix_g + mix_o) / (mix_g / grad_rate + mix_o / ov_rate)
        by_kind = {"gradient_evals_per_s": grad_rate, "overlap_evals_per_s": ov_rate,
                   "reference_mix_evals_per_s": ref_mix,
                   "reference_mix": f"{mix_g} gradients + {mix_o} overlap evals per state (one layer, SURVEY 3 S2)"}

    # the dominant kernel's roofline, from the library's timers over the timed steps (no run of its own)
    dom = max(fams, key=lambda f: fams[f]["ms"])
    fd = fams[dom]
    launches = max(fd["launches"], 1)
    avg_ms = fd["ms"] / launches
    if dom == "mps_chain":
        # fused per-state chain (k_chain).  achieved = EXECUTED FP64 flops per launch (the committed
        # PMC pass's FMA x 128 + (ADD + MUL) x 64 + MFMA MOPS x 512 per two-site update, times this
        # launch's updates) / the live launch duration.  The SURVEY 8(d) nominal count (84 n^3 for
        # the SVD of the 128 x 128 theta + 32 chi^3 theta + 32 chi^3 split, from the launch's
        # KernelTimer record) is kept beside it: the Gram path executes fewer flops than LAPACK's
        # nominal count, so the nominal rate overstates the pipes' utilisation.
        nominal = fd["flops"] / launches / (avg_ms * 1e-3) / 1e12
        upl = fd["flops"] / launches / ((84.0 * 8 + 64.0) * CHI ** 3)
        roof = {"kernel": "k_chain (fused two-site updates: theta, SVD, split)", "bound": "valu-fp64",
                "achieved": nominal, "basis": "nominal", "peak": FP64_PEAK_TFLOPS,
                "unit": "TFLOP/s", "updates_per_launch": upl,
                "nominal_achieved": nominal, "nominal_frac": nominal / FP64_PEAK_TFLOPS,
                "svd_share_of_nominal_flops": 84.0 * 8 / (84.0 * 8 + 64.0),
                "peak_note": "FP64 VALU and FP64 MFMA share one 78.6 TFLOP/s ceiling on gfx950 "
                             "(profiles/r2_fp64_pipes.txt)",
                "gram_path": dict(gram, taken_rate=gram["taken"] / max(gram["calls"], 1),
                                  taken_per_launch=gram["taken"] / launches)}
        ej = os.path.join(ROOT, "profiles", EXEC_JSON)
        if os.path.exists(ej):
            with open(ej) as fh:
                ex = json.load(fh)
            executed = ex["executed_flops_per_unit"] * upl / (avg_ms * 1e-3) / 1e12
            roof.update(achieved=executed, basis="executed (PMC)", executed_flops_per_update=ex["executed_flops_per_unit"],
                        executed_source=f"profiles/{EXEC_JSON} ({ex['formula']})",
                        pmc_wait_any_share=ex.get("wait_any_share"))
    elif dom == "mps_svd":
        jobs = fd["bytes"] / (2.0 * 4 * CHI * CHI * 16)
        achieved_flop = jobs / launches * svd_nominal_flops(2 * CHI, 2 * CHI)
        roof = {"kernel": "k_jacobi (two-site SVD)", "bound": "valu-fp64",
                "achieved": achieved_flop / (avg_ms * 1e-3) / 1e12, "peak": FP64_PEAK_TFLOPS, "unit": "TFLOP/s"}
    else:
        roof = {"kernel": dom, "bound": "hbm", "achieved": fd["bytes"] / launches / (avg_ms * 1e-3) / 1e9,
                "peak": HBM_PEAK_GBS, "unit": "GB/s"}
    roof["frac"] = roof["achieved"] / roof["peak"]
    roof["traffic"] = None
    # HBM bytes per launch of the same kernel and launch mix from the committed PMC passes
    # (tools/pmc_bench.sh: rocprofv3 FETCH_SIZE x 2 + WRITE_SIZE, MI355X_MICROARCH.md corrections)
    tj = os.path.join(ROOT, "profiles", TRAFFIC_JSON)
    want = {"mps_chain": "k_chain", "mps_svd": "k_jacobi_reg"}.get(dom)
    if want and os.path.exists(tj):
        with open(tj) as fh:
            tr = json.load(fh)
        if tr["kernel"] == want:
            roof["traffic"] = tr["traffic_bytes_per_launch"]
            roof["traffic_source"] = f"profiles/{TRAFFIC_JSON} ({tr['kernel']}, rocprofv3 PMC)"
    if want:
        roof["algorithmic_bytes_per_launch"] = fd["bytes"] / launches
    roof["avg_launch_ms"] = avg_ms
    roof["launches"] = fd["launches"]

    parity = None
    if args.full and rank == 0 and not args.no_parity and not sim:
        parity = parity_check(full, best, costs, distinct, layer_angles, shard_world, cmap, prio)
    latency = None
    if args.full and rank == 0 and world == 1 and not args.no_latency and not sim:
        latency = latency_block(distinct[0], cpu)

    if rank == 0 and sim:
        # the collective the projection leaves out: state sharding all-gathers one (best pair, score)
        # per state (16 B x S), pair sharding the whole score matrix (8 B x S x 1225); bounded by
        # RCCL's small-message latency over xGMI (COLLECTIVE_US_EST) plus the bytes at one link's
        # ~100 GB/s effective (unmeasured: the driver's SCALE run is the first multi-GPU measurement)
        ag_bytes = 16.0 * S if by_state else 8.0 * S * len(cmap)
        ag_ms = 1e-3 * COLLECTIVE_US_EST + ag_bytes / 100e9 * 1e3
        print(json.dumps({"projection": f"rank 0 of a {sim}-GPU run on one GPU (no collective)",
                          "shard": args.shard, "ms_per_step": ms_step,
                          "per_gpu_evals_per_s": evals_per_step / sim * args.steps / elapsed,
                          "projected_value": evals_per_step * args.steps / elapsed,
                          "all_gather_bytes": ag_bytes, "all_gather_ms_bound": ag_ms,
                          "ms_per_step_with_all_gather": ms_step + ag_ms,
                          "projected_value_with_all_gather": evals_per_step / (1e-3 * (ms_step + ag_ms)),
                          "breakdown_ms": {f: round(v["ms"] / args.steps, 3) for f, v in fams.items()}}))
    elif rank == 0:
        cpu_line = None
        if cpu is not None:
            g, o = cpu["gradient"]["evals_per_s"], cpu["overlap"]["evals_per_s"]
            step_mix = (len(cmap) + len(DISTANCES)) / (len(cmap) / g + len(DISTANCES) / o)
            cpu_line = {
                "value": step_mix, "unit": "evals/s", "cores": cpu["workers"], "kind": "port",
                "sample": (f"oracle port of the reference structure, {cpu['workers']} processes x 1 BLAS thread, "
                           f"{args.cpu_budget:.0f} s per kind: {cpu['gradient']['evals']} pair gradients "
                           f"(12 generators, per-pair MPS builds + dots) and {cpu['overlap']['evals']} overlap evals "
                           f"(d = 1, 2, 5, 25 round-robin, numpy SVDs), combined at the step's 1225:4 mix"),
                "gradient_evals_per_s": g, "overlap_evals_per_s": o,
                "reference_mix_evals_per_s": (mix_g + mix_o) / (mix_g / g + mix_o / o),
                # like for like: the environment form of the sweep (the device's algorithm) on the
                # same cores -- the GPU's gradient rate against the best CPU algorithm, not only
                # against the reference's per-pair structure
                "gradient_env_evals_per_s": cpu["gradient_env"]["evals_per_s"],
                "gradient_env_note": "oracle/gradients.py general_grad_of_pairs_env: whole 1225-pair sweeps",
                "host": cpu["host"],
            }
            # every physical core of the node at the measured per-process rate (an upper bound)
            pc = cpu["host"]["host_physical_cores"] / cpu["workers"]
            cpu_line["node_linear_bound"] = {
                "cores": cpu["host"]["host_physical_cores"], "value": step_mix * pc,
                "reference_mix_evals_per_s": cpu_line["reference_mix_evals_per_s"] * pc,
                "gradient_env_evals_per_s": cpu_line["gradient_env_evals_per_s"] * pc,
                "gpu_vs": value / (step_mix * pc)}
        line = {
            "metric": "overlap+gradient evals/sec, 50-qubit MPS chi=64, 1/2/4/8 MI355X",
            "value": value,
            "unit": "evals/s",
            "n_gpus": world,
            "steps": args.steps,
            "warmup": args.warmup,
            "ms_per_step": ms_step,
            "higher_is_better": True,
            "scaling": "weak",
            "vs_baseline": None,
            "dtype": "c128",
            "data": f"synthetic {args.state_kind} chi=64 Vidal MPS (seeded), random layer angles",
            "config": {
                "workload": "config3: 50-qubit chi=64 MPS; per state 1225-pair identity_resolvable gradient sweep "
                            "(sharded, RCCL all-gather, arg-max) + 4 thinly-dressed-layer overlap evals (d=1,2,5,25)",
                "n_qubits": n, "chi": CHI, "states_per_rank": B, "global_states": S,
                "pairs": len(cmap), "generators": int(len(deg)),
                "parallelism": (f"states sharded x{world} (all-gather of per-state best pair)" if by_state
                                else f"pairs sharded x{world}"),
            },
            "breakdown_ms": {f: round(v["ms"] / args.steps, 3) for f, v in fams.items()},
            "step_ms": [round(1e3 * (b - a), 3) for a, b in zip([0.0] + main_step_s[:-1], main_step_s)],
            "roofline": roof,
        }
        if args.full:
            by_kind["vs_cpu"] = ({"gradient": grad_rate / cpu_line["gradient_evals_per_s"],
                                  "gradient_like_for_like_env": grad_rate / cpu_line["gradient_env_evals_per_s"],
                                  "overlap": ov_rate / cpu_line["overlap_evals_per_s"],
                                  "reference_mix": ref_mix / cpu_line["reference_mix_evals_per_s"],
                                  "reference_mix_vs_node_linear_bound":
                                      ref_mix / cpu_line["node_linear_bound"]["reference_mix_evals_per_s"],
                                  "gradient_env_vs_node_linear_bound":
                                      grad_rate / cpu_line["node_linear_bound"]["gradient_env_evals_per_s"]}
                                 if cpu_line else None)
            line.update(by_kind=by_kind, cpu_baseline=cpu_line, parity_check=parity, latency=latency)
        print(json.dumps(line))
    if world > 1:
        dist.barrier()
        dist.destroy_process_group()


STRONG_CHI = 128
COLLECTIVE_US_EST = 50.0  # all-gather of a few KB over xGMI at 8 GPUs (RCCL small-message latency)


def strong_main(args):
    """Config 4 (BASELINE.json): 50-qubit chi = 128 candidate sweeps, strong scaling.  The global
    work is fixed: G independent sweeps (1225 pairs, identity_resolvable generators, |s> = |0..0>,
    per-state arg-max), state-sharded over the ranks (sharding.StateShard), one all-gather of the
    per-state (best pair, score).  value = G * 1225 gradient evaluations / step time (max over ranks).

    With --simulate-world N on one GPU (projection, no collective): the whole batch (T_1) and rank
    0's block of G / N (T_N) timed on the same GPU, projected speedup T_1 / (T_N + an all-gather
    estimate); and for contrast one sweep pair-sharded (sharding.PairShard): every rank's pair
    subset timed in turn, the slowest rank's time against the whole sweep."""
    import torch
    import torch.distributed as dist

    world = int(os.environ.get("WORLD_SIZE", "1"))
    rank = int(os.environ.get("RANK", "0"))
    local = int(os.environ.get("LOCAL_RANK", "0"))
    os.environ["AQC_DEVICE"] = str(local)
    torch.cuda.set_device(local)
    if world > 1:
        dist.init_process_group("nccl", device_id=torch.device("cuda", local))
    from adaptaqc_amd.device import DeviceMPS, pair_grads_batch
    from adaptaqc_amd.sharding import PairShard, StateShard, best_pairs, gather_best
    from adaptaqc_amd.utils.constants import coupling_map_fully_entangled

    n, chi, G = N_QUBITS, STRONG_CHI, args.global_states
    sim = args.simulate_world if (args.simulate_world > 1 and world == 1) else 0
    shard = StateShard(G, rank, sim or world)
    cmap = coupling_map_fully_entangled(n)
    layer, gens, deg, u0, gm = layer_inputs()
    svec = np.zeros((n, 2), complex)
    svec[:, 0] = 1.0
    prio = np.ones(len(cmap))
    distinct = [near_product_mps(n, chi, 3000 + k) for k in range(min(args.distinct, 4))]
    nres = G if sim else shard.per_rank  # resident states: the whole batch when projecting
    states = []
    for k in range(nres):
        d = DeviceMPS(n, chi, 1e-16, chi)
        d.load_aer(distinct[(shard.start + k if not sim else k) % len(distinct)])
        states.append(d)

    def barrier():
        torch.cuda.synchronize()
        if world > 1:
            dist.barrier()

    def timed(fn, k):
        barrier()
        t0 = time.perf_counter()
        for _ in range(k):
            r = fn()
        barrier()
        el = time.perf_counter() - t0
        if world > 1:
            t = torch.tensor([el], dtype=torch.float64, device="cuda")
            dist.all_reduce(t, op=dist.ReduceOp.MAX)
            el = float(t.item())
        return el / k, r

    def make_step(sts, pairs=cmap, gather=True):
        out = torch.zeros((len(sts), max(len(pairs), 1)), dtype=torch.float64, device="cuda")
        ones_t = torch.ones(max(len(pairs), 1), dtype=torch.float64, device="cuda")

        def step():
            pair_grads_batch(sts, svec, pairs, u0, gm, deg, out=out.data_ptr())
            best, score = best_pairs(out, ones_t)
            return gather_best(best, score, shard) if gather else (best, score)
        return step

    own = states[: shard.per_rank] if sim else states
    step = make_step(own, gather=not sim)
    for _ in range(args.warmup):
        step()
    t_step, (best, score) = timed(step, args.steps)
    if args.dump_outputs:
        dump_outputs(args.dump_outputs, rank, world, {"best_pair": best, "best_score": score})
    value = G * len(cmap) / (t_step if not sim else float("nan"))
    res = {"metric": "candidate-sweep gradient evals/sec, 50-qubit MPS chi=128 (config 4), strong scaling",
           "unit": "evals/s", "n_gpus": world, "steps": args.steps, "warmup": args.warmup,
           "higher_is_better": True, "scaling": "strong", "vs_baseline": None, "dtype": "c128",
           "data": "synthetic near-product chi=128 Vidal MPS (4 distinct, seeded)",
           "config": {"workload": f"config4: {G} independent 1225-pair identity_resolvable sweeps "
                                  "(|s>=|0..0>), state-sharded, per-state arg-max, one all-gather",
                      "n_qubits": n, "chi": chi, "global_states": G, "states_per_rank": shard.per_rank,
                      "parallelism": f"states sharded x{sim or world}"}}
    if not sim:
        res["value"] = value
        res["ms_per_step"] = 1e3 * t_step
        if rank == 0:
            print(json.dumps(res))
    else:
        step_all = make_step(states, gather=False)
        step_all()
        t_all, _ = timed(step_all, args.steps)
        # one sweep, pair-sharded: each rank's subset in turn, the slowest rank
        one = [states[0]]
        t_one, _ = timed(make_step(one, gather=False), args.steps)
        t_ranks = []
        for r in range(sim):
            ps = PairShard(cmap, n, r, sim)
            if ps.local_pairs:
                t_r, _ = timed(make_step(one, ps.local_pairs, gather=False), args.steps)
                t_ranks.append(t_r)
        t_coll = COLLECTIVE_US_EST * 1e-6
        res.update({
            "projection": f"rank 0 of a {sim}-GPU run on one GPU (no collective; all-gather estimated "
                          f"at {COLLECTIVE_US_EST:.0f} us)",
            "ms_global_batch_1gpu": 1e3 * t_all, "ms_rank_block": 1e3 * t_step,
            "value_1gpu": G * len(cmap) / t_all,
            "projected_value": G * len(cmap) / (t_step + t_coll),
            "projected_speedup": t_all / (t_step + t_coll),
            "single_sweep_pair_sharded": {
                "ms_whole_sweep": 1e3 * t_one, "ms_slowest_rank": 1e3 * max(t_ranks),
                "projected_speedup": t_one / (max(t_ranks) + t_coll),
                "note": "one sweep split by first qubit (segmented form, sweep_seg.h): every rank "
                        "still runs the segment products and boundary environments, the sweep's "
                        "dependent depth of ~2 sqrt(n) latency-bound GEMM launches; fewer pairs "
                        "per rank do not shorten it"},
        })
        print(json.dumps(res))
    if world > 1:
        dist.barrier()
        dist.destroy_process_group()


def parity_check(full, best, costs, distinct, layer_angles, world, cmap, prio):
    """State 0 of the last step against the oracle (outside every timed region): its 1225 gradients
    (environment form, pinned to the reference structure by the tests; 8 pairs also through the
    reference structure) and arg-max pair, and its four overlap evaluations (fused chain)."""
    from oracle import gradients as ogr, mps as M

    n = N_QUBITS
    q0 = distinct[0]
    psi = M.MPS.from_aer(q0).preprocessed()
    _, og, od, inv0 = oracle_layer()
    want = np.array(ogr.general_grad_of_pairs_env(psi, n, inv0, og, od, cmap))
    got = full[0].double().cpu().numpy()
    idx = np.random.default_rng(3).choice(len(cmap), 8, replace=False)
    want_ref = np.array(ogr.general_grad_of_pairs_ref(psi, n, inv0, og, od, [cmap[i] for i in idx], (), 1e-16, CHI))
    st = M.MPS.from_aer(q0)
    ov_err, cost_err = 0.0, 0.0
    for k, d in enumerate(DISTANCES):  # state 0's work states are the first len(DISTANCES)
        out = M.run_circuit(n, thin_layer_oracle_ops(LAYER_A, LAYER_A + d, layer_angles[k]), 1e-16, CHI, mps=st)
        c_ref = 1 - abs(M.mps_dot(out.preprocessed(), M.zero_mps(n))) ** 2
        cost_err = max(cost_err, abs(float(costs[k]) - c_ref))
    best0 = int(best[0].item())
    res = {
        "state": "state 0 (seed 1000), last timed step",
        "grad_max_abs_err_env": float(np.max(np.abs(got - want))),
        "grad_max_abs_err_ref_structure_8_pairs": float(np.max(np.abs(got[idx] - want_ref))),
        "grad_max": float(np.max(want)),
        "argmax_pair": list(cmap[best0]),
        "argmax_match": bool(best0 == int(np.argmax(want * prio))),
        "overlap_cost_max_abs_err": cost_err,
        "costs": [float(c) for c in costs[:len(DISTANCES)]],
    }
    res["ok"] = bool(res["grad_max_abs_err_env"] < 1e-9 and res["argmax_match"] and cost_err < 1e-6)
    return res


def latency_block(q0, cpu):
    """One state alone: an overlap evaluation per distance (reload + replay + save + <0|psi>), and
    one Rotoselect gate -- replace_with_best_1q_gate's 7 evaluations (cost_minimiser.py:318-342:
    the current angle, then rx / ry / rz at +-pi/2) -- as one batch from the cached MPS; medians
    over repeats, each against one evaluation of the CPU port on one core."""
    from adaptaqc_amd import _lib
    from adaptaqc_amd.device import DeviceMPS, copy_batch, apply_batch, overlap_zero_batch

    n = N_QUBITS
    src = DeviceMPS(n, CHI, 1e-16, CHI)
    src.load_aer(q0)
    rng = np.random.default_rng(11)
    cpu_ms = (cpu or {}).get("overlap", {}).get("eval_ms_by_distance", {})

    def run(ws, ops, reps=5):
        ts = []
        for _ in range(reps):
            t0 = time.perf_counter()
            copy_batch(ws, [src] * len(ws))
            apply_batch(ws, ops, sort=True)
            overlap_zero_batch(ws)
            ts.append(time.perf_counter() - t0)
        return 1e3 * float(np.median(ts[1:]))

    out = {"overlap_eval_ms": {}, "cpu_port_eval_ms_1core": cpu_ms, "speedup_vs_cpu_1core": {}}
    w = [DeviceMPS(n, CHI, 1e-16, CHI)]
    for d in DISTANCES:
        ops = [_lib.ops_array(thin_layer_ops(LAYER_A, LAYER_A + d, rng.uniform(-np.pi, np.pi, 4)))]
        out["overlap_eval_ms"][str(d)] = run(w, ops)
        if str(d) in cpu_ms:
            out["speedup_vs_cpu_1core"][str(d)] = cpu_ms[str(d)] / out["overlap_eval_ms"][str(d)]
    for d in (1, 5):
        base = rng.uniform(-np.pi, np.pi, 4)
        cands = [(tuple(THIN_AXES), base)]
        for ax in ("rx", "ry", "rz"):
            for th in (np.pi / 2, -np.pi / 2):
                c = base.copy()
                c[0] = th
                cands.append(((ax,) + tuple(THIN_AXES[1:]), c))
        ws = [DeviceMPS(n, CHI, 1e-16, CHI) for _ in cands]
        ops = [_lib.ops_array(thin_layer_ops(LAYER_A, LAYER_A + d, ang, axes)) for axes, ang in cands]
        t = run(ws, ops)
        out[f"rotoselect_gate_7_evals_ms_d{d}"] = t
        if str(d) in cpu_ms:
            out[f"rotoselect_gate_speedup_vs_cpu_1core_d{d}"] = 7 * cpu_ms[str(d)] / t
    # one candidate sweep of one state, the reference's per-layer call (gradients.py:81-122 from
    # adapt_compiler.py:839-856): 1225 pairs, host result
    from adaptaqc_amd.device import pair_grads_batch
    from adaptaqc_amd.utils.constants import coupling_map_fully_entangled

    cmap = coupling_map_fully_entangled(n)
    _, _, deg, u0, gm = layer_inputs()
    svec = np.zeros((n, 2), complex)
    svec[:, 0] = 1.0
    ts = []
    for _ in range(8):
        t0 = time.perf_counter()
        pair_grads_batch([src], svec, cmap, u0, gm, deg)
        ts.append(time.perf_counter() - t0)
    out["single_sweep_ms"] = 1e3 * float(np.median(ts[2:]))
    sref = (cpu or {}).get("sweep_ref", {})
    if sref.get("one_core_sweep_s"):  # measured: all 1225 pairs computed once, CPU time summed
        out["cpu_port_single_sweep_ms_1core"] = 1e3 * sref["one_core_sweep_s"]
        out["cpu_port_single_sweep_note"] = ("reference structure (per-pair MPS builds + dots), every pair computed "
                                             "once over the workers, their times summed")
        out["single_sweep_speedup_vs_cpu_1core"] = out["cpu_port_single_sweep_ms_1core"] / out["single_sweep_ms"]
    senv = (cpu or {}).get("gradient_env", {})
    if senv.get("one_core_sweep_s"):  # like for like: the GPU's environment algorithm on one core
        out["cpu_env_single_sweep_ms_1core"] = 1e3 * senv["one_core_sweep_s"]
        out["single_sweep_speedup_vs_cpu_env_1core"] = out["cpu_env_single_sweep_ms_1core"] / out["single_sweep_ms"]
    out["note"] = "single state on one GPU; wall time of one evaluation (or one gate's 7 as one batch, or one sweep)"
    return out


if __name__ == "__main__":
    main()
