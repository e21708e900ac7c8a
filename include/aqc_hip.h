/*
 * aqc_hip.h -- C ABI of libaqchip.so, the MI355X (gfx950) engine behind the
 * adaptaqc_amd backends.
 *
 * Every entry point replaces a specific reference call site (qiskit-community/adapt-aqc,
 * paths relative to the reference root); the arithmetic those call sites delegated to
 * qiskit-aer ~=0.16.0 and aqc_research.mps_operations runs here in hand-written HIP.
 *
 * Conventions
 *   - return value: AQC_OK (0) or a negative AQC_ERR_*; aqc_last_error() gives a
 *     thread-local message for the last failure.
 *   - complex numbers are interleaved (re, im) doubles; matrices are row-major.
 *   - gate matrices follow Qiskit: for an op on qubits (q0, q1) the row/column index is
 *     2*b1 + b0 (b0 = bit of q0).
 *   - handles own their device memory and one HIP stream; a handle is not re-entrant.
 *   - *_batch entry points take arrays of handles and run them in lock-step launches
 *     (one kernel launch serves every handle), so independent evaluations fill the GPU.
 */
#ifndef AQC_HIP_H
#define AQC_HIP_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define AQC_OK 0
#define AQC_ERR_ARG (-1)
#define AQC_ERR_HIP (-2)
#define AQC_ERR_STATE (-3)
#define AQC_ERR_UNSUPPORTED (-4)
#define AQC_ERR_NOMEM (-5)

/* One gate.  nq = 1: m[0..7] holds the 2x2 matrix; nq = 2: m[0..31] the 4x4 matrix. */
typedef struct aqc_op {
  int32_t nq;
  int32_t q0;
  int32_t q1;
  int32_t flags; /* 0: a gate; AQC_OP_KRAUS1 / AQC_OP_KRAUS2: a Kraus row of the trajectory samplers only */
  double m[32];
} aqc_op_t;

typedef struct aqc_sv_s* aqc_sv_t;
typedef struct aqc_mps_s* aqc_mps_t;
typedef struct aqc_comm_s* aqc_comm_t;

/* ---- library -------------------------------------------------------------------- */
const char* aqc_last_error(void);
int aqc_version(void);
/* Select the HIP device used by handles created afterwards (hipSetDevice). */
int aqc_init(int device);
int aqc_finalize(void);
/* Kernel-time instrumentation: accumulate HIP-event time of the named kernel family
 * ("sv_segment", "mps_svd", "grad_chain", ...) issued after the call. */
int aqc_timing_enable(int on);
int aqc_timing_query(const char* name, double* total_ms, int64_t* launches, double* bytes,
                     double* flops);
int aqc_timing_reset(void);

/* ---- statevector: replaces aer_sv_backend.py:37-59 ---------------------------- */
/* Allocate |0...0> on n qubits (Aer statevector_simulator state). */
int aqc_sv_create(int n, aqc_sv_t* out);
int aqc_sv_destroy(aqc_sv_t h);
int aqc_sv_reset(aqc_sv_t h);
int aqc_sv_copy(aqc_sv_t dst, const aqc_sv_t src);
/* Apply ops in order (aer_sv_backend.py:42-47 simulator.run(full_circuit)).  Gates are
 * fused on the host into qubit-local segments: 10-bit LDS tiles below 14 qubits, 12-bit
 * register-resident tiles (4-bit phases) from 14 qubits. */
int aqc_sv_apply(aqc_sv_t h, const aqc_op_t* ops, int nops);
/* Host planning of aqc_sv_apply only (no GPU): out[0] segments (= launches), out[1] phases
 * (register-tile path; 0 otherwise), out[2] fused gates, out[3] tile bits. */
int aqc_sv_plan(int n, const aqc_op_t* ops, int nops, int* out);
/* sv[0] (aer_sv_backend.py:29). */
int aqc_sv_amp0(aqc_sv_t h, double* re, double* im);
/* <Z_i> = p0 - p1 for all i (aer_sv_backend.py:49-59), out[n]. */
int aqc_sv_z_all(aqc_sv_t h, double* out);
/* Host copies of the full state (2^n interleaved complex). */
int aqc_sv_get(aqc_sv_t h, double* out);
int aqc_sv_set(aqc_sv_t h, const double* in);

/* ---- MPS: replaces aer_mps_backend.py:27-93 and aqc_research.mps_operations ----- */
/* |0...0> on n qubits, bond capacity chi_cap (1 ... 1024); truncation as mps_sim_with_args
 * (aer_mps_backend.py:27-42): threshold on the discarded tail sum of s^2, max_chi <= 0
 * means unlimited (bounded by chi_cap). */
int aqc_mps_create(int n, int chi_cap, double threshold, int max_chi, aqc_mps_t* out);
int aqc_mps_destroy(aqc_mps_t h);
int aqc_mps_set_truncation(aqc_mps_t h, double threshold, int max_chi);
/* Load Aer-format Vidal MPS (set_matrix_product_state, approximate_compiler.py:180-204):
 * dims[n+1] bond dims (dims[0] = dims[n] = 1); gammas: for site i, 2*dims[i]*dims[i+1]
 * complex laid out [s][l][r]; lambdas: for bond i < n-1, dims[i+1] doubles. */
int aqc_mps_set_vidal(aqc_mps_t h, const int* dims, const double* gammas, const double* lambdas);
/* Export (save_matrix_product_state): sorts qubits first.  Pass NULL to query dims. */
int aqc_mps_get_vidal(aqc_mps_t h, int* dims, double* gammas, double* lambdas);
int aqc_mps_get_dims(aqc_mps_t h, int* dims);
int aqc_mps_copy(aqc_mps_t dst, const aqc_mps_t src);
/* Batched aqc_mps_copy (dst[s] <- src[s], same n and capacity): one launch for every state --
   the per-evaluation reload of the cached MPS (reference: every cost evaluation re-runs
   full_circuit, whose first instruction is set_matrix_product_state, aer_mps_backend.py:76-78;
   the instruction is built at approximate_compiler.py:181-184). */
int aqc_mps_copy_batch(aqc_mps_t* dst, const aqc_mps_t* src, int nstates);
/* Apply ops with Aer MPS semantics (swap-left routing, lazy qubit order, two-site SVD with
 * reduce_zeros truncation) -- the replay inside mps_from_circuit (aer_mps_backend.py:76-78). */
int aqc_mps_apply(aqc_mps_t h, const aqc_op_t* ops, int nops);
int aqc_mps_apply_batch(aqc_mps_t* hs, int nstates, const aqc_op_t* const* ops, const int* nops);
/* As aqc_mps_apply_batch, then move every state back to sorted qubit order in the same schedule
   -- one evaluation's replay + save of mps_from_circuit (aer_mps_backend.py:76-78), so that a
   state's swaps back run in the same fused chain as its gates. */
int aqc_mps_apply_sort_batch(aqc_mps_t* hs, int nstates, const aqc_op_t* const* ops, const int* nops);
/* As aqc_mps_apply_sort_batch, but returns once the work is queued: the states' error flags
   (capacity, Jacobi sweep limit) are not read back -- call aqc_mps_check_batch before using the
   results.  Lets the host prepare further work (the candidate sweep) while the chain runs. */
int aqc_mps_apply_sort_batch_async(aqc_mps_t* hs, int nstates, const aqc_op_t* const* ops, const int* nops);
/* As aqc_mps_apply_batch (no sort), returning once the work is queued; flags as above.  The
   cached Rotoselect evaluator advances its prefix with it (one host wait per gate instead of three). */
int aqc_mps_apply_batch_async(aqc_mps_t* hs, int nstates, const aqc_op_t* const* ops, const int* nops);
/* Wait for the states' queued work and report their error flags (AQC_ERR_STATE etc.). */
int aqc_mps_check_batch(aqc_mps_t* hs, int nstates);
/* ---- ISL entanglement sweep (adapt_compiler.py:955-976 -> entanglement_measures.py:39-98) ----
   Two-qubit reduced density matrices for npairs pairs (pairs[2p], pairs[2p+1]), out = npairs x
   4 x 4 complex (row-major), row index 2*bit(max) + bit(min) as qiskit's partial_trace orders
   the remaining qubits.  SV: entanglement_measures.py:326-340.  MPS: the contraction of
   aqc_research.mps_operations.partial_trace (sorts qubits first); the batch version writes
   nstates x npairs x 16 complex, to device memory when out_is_device. */
int aqc_sv_pair_rdms(aqc_sv_t h, const int* pairs, int npairs, double* out);
int aqc_mps_pair_rdms(aqc_mps_t h, const int* pairs, int npairs, double* out);
int aqc_mps_pair_rdms_batch(aqc_mps_t* hs, int nstates, const int* pairs, int npairs, double* out,
                            int out_is_device);
/* Cached Rotoselect / Rotosolve (replaces the 3-7 full simulations per gate of
   cost_minimiser.py:318-368): out = 2x2 complex T[a][b] = <bra| (|a><b|)_q |ket>, so that
   <bra|V_q|ket> = sum_ab V[a][b] T[a][b] for any single-qubit V. */
int aqc_sv_transition(aqc_sv_t bra, aqc_sv_t ket, int q, double* out);
/* Measures of count 4x4 density matrices (entanglement_measures.py:245-306): method 0 =
   concurrence (EM_TOMOGRAPHY_CONCURRENCE), 1 = entanglement of formation, 2 = negativity,
   3 = log-negativity.  rdms / out in device memory when on_device. */
int aqc_entanglement_measures(const double* rdms, int count, int method, double* out, int on_device);

/* ---- shot sampling: replaces the counts of qiskit_sampling_backend.py:78-89 (Aer qasm_simulator) ----
   Random numbers are counter based, Philox4x32-10 with key = (seed & 0xffffffff, seed >> 32) and
   counter = (shot & 0xffffffff, shot >> 32, site, run & 0xffffffff); the uniform of a counter is
   u = ((x0 >> 5) * 2^26 + (x1 >> 6)) * 2^-53 from output words x0, x1.  A shot's outcome depends only
   on (seed, run, shot, site).  Neither sampler modifies the state.
   nshots outcomes of measuring every qubit of the state; out[j] = basis index (bit q = qubit q):
   the smallest k whose inclusive prefix sum of |psi_k|^2 exceeds u * total (site = 0).
   u == NULL: uniforms from (seed, run) as above; else nshots host doubles in [0,1) used instead.
   nshots < 1 (or above 2^30) or a u outside [0,1): AQC_ERR_ARG. */
int aqc_sv_sample(aqc_sv_t h, int nshots, uint64_t seed, uint64_t run, const double* u, uint64_t* out);
/* As above for an MPS (sorted to qubit order first, like every measurement): out is
   nshots x ((n+63)/64) words, bit q%64 of word q/64 = outcome of qubit q; u: NULL or nshots x n,
   [shot][site].  Site by site against the right environments (no canonical form assumed): with
   w_s = v A_i^s and p_s = Re(w_s R_{i+1} w_s^dag), bit = 1 iff u (p_0 + p_1) >= p_0, then
   v = w_bit / sqrt(p_bit).  A pending capacity or SVD flag of queued work: AQC_ERR_STATE, as in
   aqc_mps_overlap_zero. */
int aqc_mps_sample(aqc_mps_t h, int nshots, uint64_t seed, uint64_t run, const double* u, uint64_t* out);

/* ---- noisy shot sampling: quantum trajectories, replaces Aer's qasm_simulator under a NoiseModel ----
   (execute_kwargs={'noise_model': ..., 'shots': ...}, approximate_compiler.py:93).
   prog: nprog rows in order.  flags == 0: a gate, as in aqc_sv_apply.  flags == AQC_OP_KRAUS1: a
   one-qubit Kraus row on q0 (nq = 1); q1 holds the number of operators (1 .. 4) and m[8k .. 8k+7]
   the k-th 2x2 matrix.  Event index e numbers the Kraus rows in program order, E = their count.
   Per shot: psi = |0...0>, then the rows in order.  At Kraus event e: p_k = |K_k psi|^2, C_k the
   in-order inclusive sums, P = C_last; the smallest k with C_k > u_e P, and where rounding leaves
   none the last k with p_k > 0 (the statevector sampler's rule); then psi <- K_k psi / sqrt(p_k).
   After the last row out[shot] = the smallest basis index whose inclusive prefix sum of |psi|^2
   exceeds u_E total (aqc_sv_sample's rule; the sums run in a fixed order).
   choices, when not NULL: nshots x E bytes, the chosen k per event.
   u_e = sample_uniform(seed, run, shot, e) (counter (shot lo, shot hi, e, run)) for e = 0 .. E; when
   u is not NULL, u_e = u[shot (E+1) + e], host doubles in [0, 1).  An outcome depends on (seed,
   run, shot) only, not on the grid; no atomics in any reduction: two calls return the same bits.
   One workgroup carries a trajectory from start to outcome: up to 13 qubits with the state in LDS,
   from 14 to 24 on a slice of a global workspace (at most 256 workgroups and 512 MB: slow, but correct).
   AQC_ERR_ARG: n outside 1 .. 24, nshots outside 1 .. 2^30, a u outside [0, 1), a malformed row, or
   a Kraus row whose sum K^dag K differs from the identity by more than 1e-9.
   (flags & 0xff) == AQC_OP_KRAUS2: one operator of a correlated two-qubit channel on (q0, q1), the
   qubits of the gate it follows in listed order (nq = 2).  A channel of nk operators (1 .. 16) is a
   group of nk consecutive rows, row k with flags = AQC_OP_KRAUS2 | k << 8 | nk << 16 and m[0..31] =
   the 4x4 matrix K_k, index 2 b(q1) + b(q0) as a two-qubit gate row's.  A group is ONE event: E counts
   the one-qubit Kraus rows plus the groups in program order, the choice rule is the same over the
   group's operators (p_k = |K_k psi|^2 = Re Tr(K_k^dag K_k rho) with rho the 4x4 reduced density
   matrix of (q0, q1); where every K_k^dag K_k is a multiple of I within 1e-12, as for Pauli channels,
   p_k is that multiple), and choices holds k = 0 .. 15.  aqc_sv_traj_sample and
   aqc_sv_traj_pair_tomo take such rows; the MPS entry points answer AQC_ERR_ARG for them unless
   aqc_mps_traj_set_correlated has switched them on.
   AQC_ERR_ARG, before any device call, also for a malformed group: k not running 0 .. nk-1 over
   consecutive rows, nk outside 1 .. 16, differing qubits inside a group, q0 = q1 or a qubit out of
   range, an entry that is not finite, sum K^dag K off the identity by more than 1e-9. */
#define AQC_OP_KRAUS1 1
#define AQC_OP_KRAUS2 3 /* (2 is AQC_OP_MEASURE1) */
int aqc_sv_traj_sample(int n, const aqc_op_t* prog, int nprog, int nshots, uint64_t seed, uint64_t run,
                       const double* u, uint64_t* out, uint8_t* choices);

/* ---- noisy pair tomography: the nine Pauli settings of every pair under a noise model -------------
   What the reference measures when it runs a pair's nine rotated circuits under a NoiseModel
   (entanglement_measures.py:101-135), as one launch.  prog: aqc_sv_traj_sample's program (the circuit
   without its classical operations), same validation, same event numbering (E Kraus rows).
   pairs: 2 npairs ints, a != b in 0 .. n-1, either way round; used as hi = max, lo = min.
   effects: n x 3 x 2 x 4 doubles, entry [((q 3 + b) 2 + o) 4 + c] = (E00, E11, Re E01, Im E01) of the
   Hermitian 2x2 POVM effect of qubit q, basis b (0 X, 1 Y, 2 Z), outcome o: everything the reference
   appends after the circuit (sdg, h, measure, each with its error) folded into the measurement.
   ntraj = 9 nshots trajectories; trajectory t = 9 i + s serves setting s = 3 b_hi + b_lo of EVERY
   pair.  Its rows run as in aqc_sv_traj_sample; then for pair j: rho = the 4x4 RDM of the pure
   trajectory state (index 2 bit_hi + bit_lo), p_o = max(0, Re Tr[(E[hi][b_hi][o_hi] (x)
   E[lo][b_lo][o_lo]) rho]) for o = 2 o_hi + o_lo, and one outcome by aqc_multinomial_counts' rule
   (the smallest o with C_o > u P, else the last o with p_o > 0) with u = sample_uniform(seed, run, t,
   E + j).  One trajectory and one draw from that trajectory's p is one shot of the reference's
   circuit; the nine tables of a pair come from disjoint trajectories, so a pair's [9][4] table has the
   reference's joint law.  Tables of different pairs share trajectories and are correlated.
   u, when not NULL: ntraj x (E + npairs) host doubles in [0, 1), events first, then pairs.
   counts[(j 9 + s) 4 + o]: host int64, every row sums to nshots.  outcomes: NULL, or ntraj x npairs
   bytes, the drawn o.  An outcome depends on (seed, run, t) only: fewer shots give a prefix.  The
   RDM sums run in a fixed order and the counts are integer sums (integer atomics; no floating-point
   atomics): two calls return the same bits.  State placement as aqc_sv_traj_sample.
   AQC_ERR_ARG: as aqc_sv_traj_sample; n outside 2 .. 24, npairs outside 1 .. 4096, 9 nshots above
   2^30, a bad pair, or an effect that is not finite, whose pair does not sum to I within 1e-9, or
   that is not positive semidefinite within 1e-12. */
int aqc_sv_traj_pair_tomo(int n, const aqc_op_t* prog, int nprog, const int* pairs, int npairs, const double* effects,
                          int nshots, uint64_t seed, uint64_t run, const double* u, int64_t* counts, uint8_t* outcomes);

/* ---- noisy Pauli readout: every term of an operator from each trajectory -------------------------
   What the reference measures when expectation_value_of_pauli_operator runs one rotated circuit per
   term under a NoiseModel (circuit_operations_pauli_ops.py:71-103), as one launch of nshots
   trajectories.  prog, effects: as aqc_sv_traj_pair_tomo (same validation, same event numbering, E
   events).  codes: nterms x n bytes, codes[j n + q] = c_q of term j: 0 I, 1 X, 2 Y, 3 Z.
   The parity operator of a term: for each qubit q of its support S (c_q != 0),
   D_q = E[q][c_q - 1][0] - E[q][c_q - 1][1], a Hermitian 2x2 matrix; M = (x)_{q in S} D_q with the
   identity elsewhere.  (A noisy measure on a qubit outside S drops out: its two effects sum to I.
   D_q need not be a multiple of a Pauli matrix: relaxation on measure gives E0 = diag(1, g),
   E1 = diag(0, 1 - g), so D has an identity part.)
   Trajectory t runs the rows as in aqc_sv_traj_sample; then for EVERY term j: v = Re <psi_t|M_j|psi_t>,
   p+ = min(1, max(0, (1 + v) / 2)), and the outcome is 1 (parity -1) iff u >= p+, with
   u = sample_uniform(seed, run, t, E + j); when u is not NULL, u[t (E + nterms) + E + j], host doubles
   in [0, 1), events first, then terms.  One trajectory and one draw is one shot of the reference's
   circuit for that term, so plus[j] has the reference's law; different terms share trajectories and
   are correlated.
   plus[j]: host int64, the number of outcome-0 draws (the estimate is (2 plus - nshots) / nshots).
   values: NULL, or nshots x nterms doubles, v before clamping.  outcomes: NULL, or nshots x nterms
   bytes.  An outcome depends on (seed, run, t) only: fewer shots give a prefix.  Every floating-point
   sum runs in a fixed order and plus accumulates by integer atomics: two calls return the same bits.
   A factor D_q that is c sigma for a Pauli matrix sigma within 1e-14, entry by entry (noiseless
   readout, unital readout noise), costs nothing per amplitude, at any weight; a term may hold at most
   4 other ("general") factors, each doubling the loads per amplitude.
   State placement as aqc_sv_traj_sample.
   AQC_ERR_ARG, before any device call: as aqc_sv_traj_sample and the effects check of
   aqc_sv_traj_pair_tomo; n outside 1 .. 24, nterms outside 1 .. 65536, nshots outside 1 .. 2^30, a
   code above 3, an all-identity term (its value is 1: the caller answers it), a term with more than
   4 general factors. */
int aqc_sv_traj_pauli_counts(int n, const aqc_op_t* prog, int nprog, const uint8_t* codes, int nterms,
                             const double* effects, int nshots, uint64_t seed, uint64_t run, const double* u,
                             int64_t* plus, double* values, uint8_t* outcomes);

/* ---- noisy shot sampling above 24 qubits: quantum trajectories on the MPS engine -----------------
   (Aer's qasm_simulator with method="matrix_product_state" under a NoiseModel.)
   prog: aqc_sv_traj_sample's program.  Per shot: an MPS |0...0> of capacity chi_cap with the
   truncation (threshold, max_chi) of aqc_mps_create, the gate rows as the engine's two-site updates
   (swap-left routing, one-qubit gates deferred), each Kraus row at the orthogonality centre, then the
   qubits sorted and measured one by one, q = 0 .. n-1.  The schedule keeps the centre on the host (two
   integers, independent of the state) and moves it by identity-gate two-site updates, so the one-site
   reduced density matrix rho[s][s'] = sum_{l,r} lambda_p[l]^2 lambda_{p+1}[r]^2 Gamma_p^s[l][r]
   conj(Gamma_p^s'[l][r]) is exact wherever it is used: the law of the counts is the channel's.
   Kraus event e: p_k = Re Tr(K_k^dag K_k rho) and aqc_sv_traj_sample's choice rule with u_e, then
   Gamma^s <- sum_s' K_k[s][s'] / sqrt(p_k) Gamma^s' (a pending one-qubit gate P of that qubit is
   absorbed first, K_k <- K_k P).  Measurement of qubit q: bit = [u_{E+q} (rho00 + rho11) >= rho00]
   (aqc_mps_sample's rule), then the projection.
   out: nshots x ((n+63)/64) words in aqc_mps_sample's format.  choices: NULL, or nshots x E bytes.
   u_i = sample_uniform(seed, run, shot, i) for i = 0 .. E+n-1 (events first, then the qubits); when u
   is not NULL, u_i = u[shot (E+n) + i], host doubles in [0, 1).
   The shots run in batches of B trajectories held as B internal MPS handles: B = min(nshots, 256,
   what 4 GiB of device memory hold of them, at least 1).  A shot's result depends on (seed, run, shot)
   only, not on B; no atomics in any reduction: two calls return the same bits.
   A correlated group (AQC_OP_KRAUS2 rows; only under aqc_mps_traj_set_correlated(1 or 2), else
   AQC_ERR_ARG) is one event with the semantics of aqc_sv_traj_sample: p_k = Re Tr(K_k^dag K_k rho) with
   rho the 4x4 RDM of (q0, q1), the constant multiple where every K_k^dag K_k is one (by the same host
   arithmetic), the same choice rule, choices k = 0 .. 15, the same check of malformed groups before any
   device call.  It runs one of two ways.  General: the two qubits are routed to adjacent sites like a
   gate's, the pending one-qubit gates folded in (K_k <- K_k (P_q1 (x) P_q0)), the centre brought to the
   two sites; theta of the two sites is contracted once, rho_{oo'} = sum_{l,r} theta_o[l][r]
   conj(theta_o'[l][r]) (o = 2 s1 + s2) summed in fixed slices of 1024 (l, r) positions, the operator
   chosen and K_k / sqrt(p_k) applied to theta in place, and theta' split by the engine's SVD as after
   any two-site update; the centre then stands on the two sites.  Product-unitary -- every K_k a scalar times A_k (x) B_k with both factors
   unitary within 1e-12 (every Pauli channel, the two-qubit depolarizing error): the weights are
   constants and the operators one-site unitaries, so k is drawn from the constants and the chosen A_k,
   B_k (pending gates folded in) act on the two sites where the qubits sit, adjacent or not, with no
   routing, no centre move and no SVD.
   AQC_ERR_ARG as aqc_sv_traj_sample (n < 1, a malformed row, sum K^dag K off the identity by more
   than 1e-9, a u outside [0, 1), nshots outside 1 .. 2^30).  AQC_ERR_STATE ("capacity (chi_cap)
   exceeded") when any trajectory outgrows chi_cap: no part of the output is valid then. */
int aqc_mps_traj_sample(int n, int chi_cap, double threshold, int max_chi, const aqc_op_t* prog, int nprog,
                        int nshots, uint64_t seed, uint64_t run, const double* u, uint64_t* out, uint8_t* choices);
/* Host planning of aqc_mps_traj_sample only (no GPU): the site-level schedule every shot runs, the
   final sort and the measurement sweep included, as up to sched_cap rows in sched (NULL with
   sched_cap 0 to count only).  q0 is the site.  flags == 0: a unitary row -- nq = 2: a two-site update
   on sites (q0, q0 + 1) = q1, m the 4x4 matrix in site order (index 2 s_q0 + s_{q0+1}) with the
   pending one-qubit gates folded in (routing swaps and centre moves are such rows, a centre move
   carrying the identity); nq = 1: a flushed one-qubit gate.  (flags & 0xff) == AQC_OP_KRAUS1: a Kraus
   row, q1 operators in m after folding, the event index in flags >> 8.  flags == AQC_OP_MEASURE1: the
   measurement of qubit q1 (= q0, the qubits being sorted), m = {|0><0|, |1><1|}.
   (flags & 0xff) == AQC_OP_KRAUS2 (under aqc_mps_traj_set_correlated): a group's event as nk
   consecutive rows, nq = 2, flags = AQC_OP_KRAUS2 | k << 8 | nk << 16, q0 < q1 the two sites and m the
   folded K_k in site order (index 2 s_q0 + s_q1).  A general group: q1 = q0 + 1, and the event counts as
   a two-site update of those sites.  A product-unitary group adds bit 24 to flags; its sites need not be
   adjacent and it moves neither the centre nor a qubit.  Events are numbered in row order, a group
   taking one number.
   counts[7]: gate updates, routing / sorting swap updates, centre-move updates, one-site unitary
   rows, Kraus events (one-qubit rows and groups, one per group), measurement rows, all rows. */
#define AQC_OP_MEASURE1 2
int aqc_mps_traj_plan(int n, const aqc_op_t* prog, int nprog, int* counts, aqc_op_t* sched, int sched_cap);
/* Debugging: forces the batch size B of aqc_mps_traj_sample, aqc_mps_traj_pair_tomo and
   aqc_mps_traj_pauli_counts (1 .. 4096; 0 restores the default). */
int aqc_mps_traj_set_batch(int batch);
/* Correlated two-qubit groups (AQC_OP_KRAUS2 rows) on the MPS trajectory engine, process-wide like
   aqc_mps_traj_set_batch.  0 (default): aqc_mps_traj_plan, aqc_mps_traj_tomo_plan, aqc_mps_traj_sample,
   aqc_mps_traj_pair_tomo and aqc_mps_traj_pauli_counts answer AQC_ERR_ARG for such a row.  1: they take
   groups.  2: as 1 with every group on the general path, product-unitary ones included (debugging: a
   second route to the same outcomes).  AQC_ERR_ARG outside 0 .. 2. */
int aqc_mps_traj_set_correlated(int mode);

/* ---- noisy pair tomography above 24 qubits: aqc_sv_traj_pair_tomo on the MPS engine ---------------
   The semantics of aqc_sv_traj_pair_tomo (pairs, effects, settings, draw rule, u layout, counts and
   outcomes: see there) on the engine of aqc_mps_traj_sample.  ntraj = 9 nshots trajectories, each an
   MPS |0...0> of capacity chi_cap with the truncation (threshold, max_chi); trajectory t = 9 i + s
   serves setting s of EVERY pair.  A trajectory runs aqc_mps_traj_sample's schedule without the
   measurement sweep: gate rows, Kraus rows at the tracked centre (same event numbering, choice rule
   and folding K_k <- K_k P; correlated groups as there, under aqc_mps_traj_set_correlated), then the
   flush of pending one-qubit gates and the sort.  For pair j, rho is
   the 4x4 RDM of the trajectory's MPS (index 2 bit_hi + bit_lo) by the full contraction of
   aqc_mps_pair_rdms_batch, which assumes no canonical form (a Kraus row breaks Vidal form);
   p_o = max(0, Re Tr[(E[hi][b_hi][o_hi] (x) E[lo][b_lo][o_lo]) rho]), and one outcome by
   aqc_multinomial_counts' rule with u = sample_uniform(seed, run, t, E + j), or u[t (E + npairs) + E + j]
   when u is not NULL.  P is the sum of the four p_o, so a truncated trajectory (Tr rho < 1) needs no
   renormalisation.
   The trajectories run in batches of B handles and are read out R at a time: R = min(ntraj, 16, what
   2 GiB hold of the RDM sweep's per-state workspace, at least 1), B = min(ntraj, 256, what 4 GiB less
   that workspace hold of handles, at least 1); under a batch that aqc_mps_traj_set_batch forces, R is
   what that batch leaves.  The count table accumulates on the device (integer atomics; no
   floating-point atomics, every sum in a fixed order) and is copied back once.  An outcome depends on
   (seed, run, t) only -- not on B, the readout sub-batch or nshots (fewer shots give a prefix): two
   calls return the same bits.
   AQC_ERR_ARG: as aqc_sv_traj_pair_tomo with n in 2 .. 4096, and chi_cap outside 1 .. 1024.
   AQC_ERR_STATE ("capacity (chi_cap) exceeded") when a trajectory outgrows chi_cap: no output is valid
   then. */
int aqc_mps_traj_pair_tomo(int n, int chi_cap, double threshold, int max_chi, const aqc_op_t* prog, int nprog,
                           const int* pairs, int npairs, const double* effects, int nshots, uint64_t seed, uint64_t run,
                           const double* u, int64_t* counts, uint8_t* outcomes);
/* aqc_mps_traj_plan for aqc_mps_traj_pair_tomo's schedule: no measurement rows (counts[5] = 0), the
   last row belongs to the final sort or the flush. */
int aqc_mps_traj_tomo_plan(int n, const aqc_op_t* prog, int nprog, int* counts, aqc_op_t* sched, int sched_cap);
/* Debugging: forces the number of states per readout sweep of aqc_mps_traj_pair_tomo (the RDM sweep) and
   of aqc_mps_traj_pauli_counts (environments, chains, draw) (1 .. 4096, at most the batch; 0 restores
   the default). */
int aqc_mps_traj_set_readout_batch(int batch);

/* ---- the noisy Pauli readout above 24 qubits: aqc_sv_traj_pauli_counts on the MPS engine ----------
   The semantics of aqc_sv_traj_pauli_counts (prog, codes, effects, event numbering, u layout, plus,
   values and outcomes: see there) on the engine of aqc_mps_traj_pair_tomo.  Trajectory t is an MPS
   |0...0> of capacity chi_cap with the truncation (threshold, max_chi) and runs
   aqc_mps_traj_pair_tomo's schedule: gate rows, Kraus rows at the tracked centre, the flush, the sort,
   no measurement sweep.  For EVERY term j, M_j = (x)_{q in S} D_q with D_q = E[q][c_q - 1][0] -
   E[q][c_q - 1][1], and v = Re <psi_t|M_j|psi_t> by a transfer chain over the term's support lo..hi
   between the identity environments L_lo and R_{hi+1}, which assume no canonical form:
     E = L_lo;  E'[b'][k'] = sum_{s,t} D_i[s][t] conj(A_s[b][b']) E[b][k] A_t[k][k'] for i = lo..hi
   (D_i = I on a site outside S);  v = Re sum E[b][k] R_{hi+1}[k][b].
   w = <psi_t|psi_t> by the route of aqc_mps_pauli_expect's all-identity term (L_0, one identity step,
   R_1).  Neither is divided by the other: p+ = max(0, (w + v) / 2), p- = max(0, (w - v) / 2), and the
   outcome is 1 (parity -1) iff u (p+ + p-) >= p+, so a truncated trajectory (w < 1) needs no
   renormalisation.  u = sample_uniform(seed, run, t, E + j); when u is not NULL,
   u[t (E + nterms) + E + j], host doubles in [0, 1), events first, then terms.
   plus[j]: host int64, the number of outcome-0 draws.  values: NULL, or nshots x nterms doubles, v.
   norms: NULL, or nshots doubles, w.  outcomes: NULL, or nshots x nterms bytes.
   A general factor costs what a Pauli one does: there is no limit on them.
   The trajectories run in batches of B handles and are read out R at a time (the environments of R
   states, one chain per (term, state), one draw per (state, term)): R = min(B, 128, what half of 4 GiB
   less the chains' workspace (at most 512 MiB) hold of the environments, at least 1), B = min(nshots,
   256, what is left of it hold of handles, at least 1); aqc_mps_traj_set_batch and aqc_mps_traj_set_readout_batch force them.  An
   outcome depends on (seed, run, t) only -- not on B, R or nshots (fewer shots give a prefix).  Every
   floating-point sum runs in a fixed order and plus accumulates on the device by integer atomics only
   (copied back once): two calls return the same bits.
   AQC_ERR_ARG, before any device call: n outside 1 .. 4096, chi_cap outside 1 .. 1024, nterms outside
   1 .. 65536, nshots outside 1 .. 2^30, a code above 3, an all-identity term, a malformed row, a
   correlated (AQC_OP_KRAUS2) row unless aqc_mps_traj_set_correlated allows it (then a malformed group,
   as aqc_mps_traj_sample), the effects check of aqc_sv_traj_pair_tomo, a u outside [0, 1).
   AQC_ERR_STATE ("capacity (chi_cap) exceeded") when a trajectory outgrows chi_cap: no output is valid
   then. */
int aqc_mps_traj_pauli_counts(int n, int chi_cap, double threshold, int max_chi, const aqc_op_t* prog, int nprog,
                              const uint8_t* codes, int nterms, const double* effects, int nshots, uint64_t seed,
                              uint64_t run, const double* u, int64_t* plus, double* values, double* norms,
                              uint8_t* outcomes);

/* ---- density-matrix engine: replaces Aer's method="density_matrix" under a NoiseModel ---------------
   rho of n qubits, 1 <= n <= 13, as 4^n interleaved complex128 in device memory: entry (r, c) at index
   r + (c << n), r and c little-endian in the qubits as the statevector's index (n = 13 is 1 GiB).  One
   deterministic evolution gives exactly what the trajectory samplers estimate: the noisy cost 1 - rho_00,
   every pair's RDM, every Pauli term and the outcome distribution.  No atomics, no uniforms: two calls
   give the same bits.
   aqc_dm_create: rho = |0...0><0...0|; aqc_dm_reset restores it.  AQC_ERR_ARG for n outside 1 .. 13. */
typedef struct aqc_dm_s* aqc_dm_t;
int aqc_dm_create(int n, aqc_dm_t* out);
int aqc_dm_destroy(aqc_dm_t h);
int aqc_dm_reset(aqc_dm_t h);
/* prog: aqc_sv_traj_sample's program, unchanged.  A gate row is rho <- U rho U^dag, an AQC_OP_KRAUS1 row
   rho <- sum_k K_k rho K_k^dag, an AQC_OP_KRAUS2 group the same sum over its rows (4x4 index 2 b(q1) +
   b(q0)).  Rows on the same one or two qubits fold into one step, steps into segments of at most 6 qubits,
   one launch per segment (aqc_dm_plan).  Returns when the evolution is done.
   AQC_ERR_ARG, before any device call, as aqc_sv_traj_sample: a qubit out of range, a malformed Kraus row
   or group, sum K^dag K off the identity by more than 1e-9, AQC_OP_MEASURE1 or unknown flags. */
int aqc_dm_apply(aqc_dm_t h, const aqc_op_t* prog, int nprog);
/* Host planning of aqc_dm_apply only (no GPU).  counts[0] = segments (= launches), [1] = steps, [2] = the
   program rows folded into them, [3] = the index bits of the largest tile (at most 12).  steps: NULL, or
   room for cap steps, filled in execution order.  A step acts on the 4 (nq = 1) or 16 (nq = 2) entries of
   rho that share every other index bit, at the local index j = r_q0 + 2 c_q0, or (r_q0 + 2 r_q1) +
   4 (c_q0 + 2 c_q1).  kind 0, unitary: m[0..7] / m[0..31] = U (2x2, or 4x4 with index 2 b(q1) + b(q0)),
   X <- U X U^dag.  kind 1, superoperator: m[0..31] / m[0..511] = S (4x4 / 16x16, row-major, (re, im)),
   S[j', j] = sum_k K[r', r] conj(K[c', c]), x <- S x.  Steps of one segment act in the order listed;
   steps on disjoint qubits may have been reordered against the program.  AQC_ERR_ARG as aqc_dm_apply
   and for n outside 1 .. 13. */
typedef struct aqc_dm_step {
  int32_t kind;
  int32_t nq;
  int32_t q0;
  int32_t q1;
  int32_t segment;
  int32_t pad[3];
  double m[512];
} aqc_dm_step_t;
int aqc_dm_plan(int n, const aqc_op_t* prog, int nprog, int* counts, aqc_dm_step_t* steps, int cap);
/* X <- Lambda^dag(X), Lambda the map of aqc_dm_apply for the same rows (the Heisenberg picture): the
   whole program in reverse, a gate row as X <- U^dag X U, a Kraus row or group as X <- sum_k K_k^dag X K_k.
   The forward plan run backwards: its segments in reverse order, each segment's steps in reverse order,
   every U replaced by U^H and every S by S^H (the adjoint of x <- S x under Tr(A^H B), in the same local
   index); the tiles, records and kernel are aqc_dm_apply's.  Tr(X^H Lambda(rho)) = Tr(Lambda^dag(X)^H rho).
   X is any complex matrix (aqc_dm_set).  Argument checks as aqc_dm_apply. */
int aqc_dm_apply_adjoint(aqc_dm_t h, const aqc_op_t* prog, int nprog);
/* aqc_dm_plan for aqc_dm_apply_adjoint: the steps in the order it executes them, with the matrices it
   uses.  The counts equal the forward plan's. */
int aqc_dm_plan_adjoint(int n, const aqc_op_t* prog, int nprog, int* counts, aqc_dm_step_t* steps, int cap);
/* The host copy of rho: 2 x 4^n doubles. */
int aqc_dm_get(aqc_dm_t h, double* out);
/* Uploads 2 x 4^n doubles in aqc_dm_get's layout: any complex matrix, Hermitian or not. */
int aqc_dm_set(aqc_dm_t h, const double* in);
/* The matrix diag(d): zero everywhere but the 2^n real diagonal entries d[k] (an observable that is
   diagonal in the computational basis, for aqc_dm_apply_adjoint). */
int aqc_dm_set_diag(aqc_dm_t h, const double* d);
/* dst <- src on the device.  AQC_ERR_ARG when the qubit counts differ. */
int aqc_dm_copy(aqc_dm_t dst, aqc_dm_t src);
/* out = T, 4x4 complex, row-major as (re, im): T[j', j] = sum_o conj(A[j', o]) B[j, o], with j = r_q + 2 c_q
   the local index of qubit q (bit q and bit n + q of the entry index) and o the other 2n - 2 index bits.
   For any superoperator S on qubit q, Tr(A^H (S_q (x) id)(B)) = sum_{j', j} S[j', j] T[j', j]: with
   A = Lambda_S^dag(O) and B the state before a one-qubit gate, every candidate gate's cost from one scan.
   sum_j T[j, j] = Tr(A^H B).  A and B are read once each; the scan is spread over workgroups (one when
   4^(n-1) <= 256), each writing a partial in a fixed order, and a second pass adds the partials in order:
   no atomics, two calls give the same bits.  a == b is allowed.  AQC_ERR_ARG: q outside 0 .. n-1, different
   qubit counts. */
int aqc_dm_transition(aqc_dm_t a, aqc_dm_t b, int q, double* out);
/* out[0] = Re rho_00, out[1] = Re Tr rho. */
int aqc_dm_trace0(aqc_dm_t h, double* out);
/* Writes a_k = sqrt(max(0, Re rho_kk)) into an n-qubit statevector: aqc_sv_sample then draws shots from
   the diagonal by its inverse-CDF rule, aqc_sv_z_all gives every <Z>, aqc_sv_get the probabilities'
   roots.  AQC_ERR_ARG when sv has another qubit count. */
int aqc_dm_diag_sv(aqc_dm_t h, aqc_sv_t sv);
/* out[t] = Re Tr(M_t rho).  codes: nterms x n bytes as aqc_sv_traj_pauli_counts (no all-identity term).
   effects NULL: M_t is the Pauli string.  Otherwise effects is aqc_sv_traj_pair_tomo's [n][3][2][4] table
   and M_t = (x)_{q in support} (E_q[+] - E_q[-]), folded as aqc_sv_traj_pauli_counts folds it, with any
   number of general factors (a term reads 2^n 2^ng entries).  Not divided by Tr rho.  One workgroup per
   term, fixed summation order.  AQC_ERR_ARG: nterms outside 1 .. 65536, a code above 3, an all-identity
   term, the effects check of aqc_sv_traj_pair_tomo. */
int aqc_dm_pauli_expect(aqc_dm_t h, const uint8_t* codes, int nterms, const double* effects, double* out);
/* out[p] = the 4x4 RDM of pair p (16 complex, row-major), conventions of aqc_sv_pair_rdms: index
   2 bit_hi + bit_lo, hi the pair's larger qubit; the sum over the 2^(n-2) values of the other qubits in a
   fixed order, one workgroup per pair.  n >= 2, at most 4096 pairs. */
int aqc_dm_pair_rdms(aqc_dm_t h, const int* pairs, int npairs, double* out);
/* out[p] = the 4x4 environment of pair p in aqc_dm_pair_rdms's layout: with r the other qubits' row bits
   and r' their column bits,
     R[a][b] = sum_{r, r'} rho[(a, r), (b, r')] prod_{q not in p} E_q[r'_q, r_q] = Tr_rest((1 (x) E_rest) rho),
   so that Tr(((x)_q E_q) (Lambda (x) id)(rho)) = Tr((E_hi (x) E_lo) Lambda(R)) for any channel Lambda on the
   pair: every candidate gate on the pair, with its errors, in front of a product measurement is priced on
   the host from R.  effects: n x 4 doubles, (E00, E11, Re E01, Im E01) of qubit q's Hermitian effect (the
   entries of a pair's own qubits are ignored), or NULL for identity effects (R is then the RDM).  r' runs
   only over the qubits whose effect has a nonzero off-diagonal: ng of them cost a pair 16 x 2^(n-2+ng)
   entries, all-diagonal effects the bytes of aqc_dm_pair_rdms.  A pair is spread over up to 256 workgroups
   (256 items each at first), which write partials that a second pass adds in order: no atomics, two
   calls give the same bits.  rho is any matrix (aqc_dm_set) and is not changed.  n >= 2, at most 4096
   pairs; AQC_ERR_ARG also for an effect that is not finite. */
int aqc_dm_pair_envs(aqc_dm_t h, const int* pairs, int npairs, const double* effects, double* out);
/* aqc_dm_transition for pairs.  out[p] = T, 16x16 complex, row-major (j' major) as (re, im):
     T[j', j] = sum_o conj(A[j', o]) B[j, o],   j = (r_lo + 2 r_hi) + 4 (c_lo + 2 c_hi),
   lo / hi the smaller / larger qubit of pair p in whatever order it is listed (index bits lo, hi, n + lo,
   n + hi of the entry), o the other 2n - 4 index bits.  For any two-qubit superoperator S at that index (an
   aqc_dm_plan step on (lo, hi)), Tr(A^H (S (x) id)(B)) = sum_{j', j} S[j', j] T[j', j]: with A a cost observable
   pulled back through everything behind a candidate layer (aqc_dm_apply_adjoint) and B the state in front of
   it, every candidate layer on the pair is priced on the host, whatever follows it.  Summing T over the
   partner's equal indices gives aqc_dm_transition's T of either qubit.
   Per pair a 16 x 16 x 4^(n-2) complex product on the FP64 matrix cores; both matrices are read once per
   pair.  A pair is spread over aqc_dm_pair_transitions_plan's workgroups, each adding its waves' tiles in order,
   and a second pass adds a pair's workgroups in order: no atomics, two calls give the same bits.  a == b is
   allowed; neither is changed.  AQC_ERR_ARG: different qubit counts, n < 2, a qubit out of range, a pair of
   equal qubits, more than 4096 pairs. */
int aqc_dm_pair_transitions(aqc_dm_t a, aqc_dm_t b, const int* pairs, int npairs, double* out);
/* Host only (no GPU): *split = the workgroups aqc_dm_pair_transitions spreads one pair over for npairs pairs
   of n qubits: 1 while 4^(n-2) <= 256, then 256 values of o a workgroup up to 256 workgroups (4 at n = 7),
   halved while split x npairs exceeds 8192.  AQC_ERR_ARG: n outside 2 .. 13, npairs outside 1 .. 4096. */
int aqc_dm_pair_transitions_plan(int n, int npairs, int* split);

/* ---- Pauli-string expectation values: replaces circuit_operations_pauli_ops.py:60-100 -------------
   (expectation_value_of_pauli_operator, which runs one rotated circuit per term).
   out[t] = Re <psi| P_t |psi>,  P_t = i^{popcount(x&z)} X^{x} Z^{z}  (a qubit set in both masks is Y);
   bit q of a mask = qubit q.  A mask bit at or above n: AQC_ERR_ARG.  Does not modify the state.
   All terms go in one launch; sums run in a fixed order (no atomics): the same state gives the
   same bits. */
int aqc_sv_pauli_expect(aqc_sv_t h, const uint64_t* xmask, const uint64_t* zmask, int nterms, double* out);
/* ---- operator apply and vector operations: what a Krylov ground-state solver needs (replaces the
   host eigensolver behind hamiltonians.py:80-85, calculate_ground_state) ---------------------------
   out = sum_t c_t P_t in, P_t as above, c_t = coeff[2t] + i coeff[2t+1]:
   out[j] = sum_t c_t i^{ny_t} (-1)^{popcount((j ^ x_t) & z_t)} in[j ^ x_t].  nterms == 0: out = 0.  An
   all-identity term (x = z = 0) is an offset c in.  The terms are grouped by x mask (groups in order of
   first appearance, terms of a group in input order); an amplitude is the sum over the groups in that
   order of (sum of the group's +-c_t i^{ny_t} in term order) times in[j ^ X]; a group of more than 383
   terms is cut into runs of 383 that are summed like groups.  No atomics: the same inputs give the
   same bits.  in is not modified.
   AQC_ERR_ARG, with out untouched: a null handle, in == out, different qubit counts, a mask bit at or
   above n, a coefficient that is not finite, nterms outside 0 .. 2^20. */
int aqc_sv_pauli_apply(aqc_sv_t in, aqc_sv_t out, const uint64_t* xmask, const uint64_t* zmask, const double* coeff,
                       int nterms);
/* out2 = (re, im) of sum_k conj(a_k) b_k, summed in a fixed order (a thread's terms in index order, the
   wave, the waves in order, then the workgroups' partials in order).  a == b is allowed. */
int aqc_sv_dot(aqc_sv_t a, aqc_sv_t b, double* out2);
/* y <- (ar + i ai) y + (br + i bi) x.  b == 0: x is not read and may be NULL (a pure scale).
   AQC_ERR_ARG: a null y, x == y, a null x with b != 0, different qubit counts, a coefficient that is not
   finite. */
int aqc_sv_axpby(aqc_sv_t y, double ar, double ai, aqc_sv_t x, double br, double bi);
/* codes: nterms x n bytes, codes[t*n + q] in {0 I, 1 X, 2 Y, 3 Z} for qubit q; out: nterms doubles
   (batch: nstates x nterms).  The states are sorted to qubit order first, as every measurement.
   <psi|P|psi> is NOT divided by <psi|psi>: same convention as aqc_mps_z_all, so a truncated state
   gives the same number z_all gives for a single Z, and the all-identity term gives <psi|psi>.
   Pending capacity / SVD flags of queued work: AQC_ERR_STATE, as aqc_mps_overlap_zero.
   Batch: all states need the same n and capacity (AQC_ERR_ARG otherwise).  A code above 3: AQC_ERR_ARG.
   The identity environments of every bond come from the chains of aqc_mps_z_all_batch; each
   (term, state) then runs its support's transfer steps in one workgroup of its own (no
   synchronisation between workgroups), so at capacity 1024 a long string is slow but correct. */
int aqc_mps_pauli_expect(aqc_mps_t h, const uint8_t* codes, int nterms, double* out);
int aqc_mps_pauli_expect_batch(aqc_mps_t* hs, int nstates, const uint8_t* codes, int nterms, double* out);

/* ---- two-site DMRG ground states of a Pauli sum on the MPS engine (dmrg.hip): the route of
   calculate_ground_state above a statevector's reach ------------------------------------------------
   H = sum_t c_t P_t with real c_t; codes as aqc_mps_pauli_expect takes them.  At bond b (sites b, b + 1,
   0 <= b <= n - 2) a term with support lo..hi is closed left (hi < b: summed into one matrix LH_b),
   closed right (lo > b + 1: into RH_b), local (b <= lo, hi <= b + 1: into one 4 x 4 matrix h_b), open
   (anything else: a record of its own) or, without support, a constant kept on the host.
   aqc_mps_dmrg_plan needs no GPU.  totals[8]: records over all bonds, the most records of one bond,
   stored environment matrices, their bytes at chi_cap, the bytes of scratch (W of every record, the
   Krylov basis, the environment steps' panels), the record limit of one bond, the byte budget of
   environments plus scratch, the number of identity terms.  bonds (null, or (n - 1) x 7): records, closed
   left terms, closed right terms, local terms, open records, stored left environments of open terms,
   stored right ones.  records (null, or records_cap >= totals[0] rows of 4): bond, kind (0 LH, 1 RH,
   2 local, 3 open), term (kind 3, else -1), flags (bit 0: a stored left environment, bit 1: a stored
   right one); a bond's records in the order LH, RH, local, then its open terms in input order.  classes
   (null, or (n - 1) x nterms bytes): 0 closed left, 1 closed right, 2 local, 3 open, 4 identity.
   AQC_ERR_ARG: n outside 2 .. 4096, nterms outside 1 .. 2^20, chi_cap outside 1 .. 1024, krylov_dim outside
   2 .. 16, a code above 3, a coefficient that is not finite, a bond with more records than the limit,
   environments plus scratch above the budget (the last two name their numbers). */
typedef struct aqc_dmrg_s* aqc_dmrg_t;
int aqc_mps_dmrg_plan(int n, const uint8_t* codes, const double* coeffs, int nterms, int chi_cap, int krylov_dim,
                      int64_t* totals, int* bonds, int* records, int records_cap, uint8_t* classes);
/* A DMRG handle on `mps` (which it does not own and which must outlive it): the environments, the Krylov
   scratch and the record tables at the state's capacity.  AQC_ERR_ARG as the plan; the MPS is not
   touched.  The handle follows the state through its own sweeps and refuses it (AQC_ERR_STATE) after any
   other change. */
int aqc_dmrg_create(aqc_mps_t mps, const uint8_t* codes, const double* coeffs, int nterms, int krylov_dim,
                    aqc_dmrg_t* out);
/* One sweep: two-site updates of the bonds 0 .. n - 2 left to right, then back.  An update forms theta,
   replaces it with the lowest Ritz vector of a Lanczos iteration of krylov_dim steps (full
   reorthogonalisation; every scalar on the device; ended early at beta <= 256 eps S, S = sum |c_t|, or
   when the space is exhausted) on the bond's effective Hamiltonian, and hands it to the engine's SVD,
   truncation (the state's max_chi and threshold), renormalisation and split; the environment step
   for the next bond follows.  The first sweep first sorts the qubits and runs identity updates in both
   directions (the gauge), then builds every right environment.  Nothing waits on the host between
   bonds.  bond_energies: 2 (n - 1) Ritz values in update order.  Every sum runs in a fixed order: the
   same state and operator give the same bits. */
int aqc_dmrg_sweep(aqc_dmrg_t h, double* bond_energies);
int aqc_dmrg_destroy(aqc_dmrg_t h);

/* ---- shot-based pair tomography: replaces the per-pair circuits of entanglement_measures.py:101-135
   (perform_quantum_tomography) and :138-250 (measure_concurrence_lower_bound) ----
   Each of those circuits measures two qubits, so its counts are a multinomial draw that the pair's
   4x4 reduced density matrix fixes: the state is simulated once, the RDMs come from the pair-RDM
   entry points above, and counts, fit and measure of every pair follow in a few launches.
   Conventions: pair (a, b) as hi = max, lo = min; RDM index 2 bit_hi + bit_lo; basis codes 0 X, 1 Y,
   2 Z; setting s = 3 b_hi + b_lo; outcome o = 2 o_hi + o_lo with 0 the +1 eigenstate -- X: (|0> +- |1>)
   / sqrt 2, Y: (|0> +- i|1>) / sqrt 2 (which sdg then h maps onto |0>, |1>), Z: |0>, |1>.
   rdms / out (and counts / out_rdms of aqc_tomo_fit) in device memory when on_device. */
/* out[(pair 9 + s) 4 + o] = max(0, <v|rho|v>), v the product eigenvector of (s, o).  Not
   renormalised (a truncated MPS has Tr rho < 1; the draw divides by the total). */
int aqc_pair_tomo_probs(const double* rdms, int npairs, double* out, int on_device);
/* out[3 pair + c]: the key probabilities of the three two-copy circuits, c = 0: P("1111") =
   (1 - Tr rho_1^2 - Tr rho_2^2 + Tr rho_12^2) / 4, 1: P("0011") = (1 - Tr rho_1^2) / 2, 2: P("1100") =
   (1 - Tr rho_2^2) / 2, each clamped at 0; rho_1 / rho_2: the marginal of the pair's lower / higher qubit. */
int aqc_concurrence_bound_probs(const double* rdms, int npairs, double* out, int on_device);
/* counts[job K + k] (int64) of nshots draws from job's K probabilities (2 <= K <= 16), nshots in
   1 .. 2^30.  Job j's shot t uses sample_uniform(seed, run, t, j) (counter (t lo, t hi, j, run)), or
   u[t njobs + j] when u is not null (the layout of aqc_sample_uniforms(seed, run, nshots, njobs)).
   Rule, with C_k the in-order inclusive sums and P = C_{K-1}: the smallest k with C_k > u P; where
   rounding leaves none, the last k with p_k > 0 (the statevector sampler's rule).  A negative or
   non-finite probability, or P = 0: AQC_ERR_ARG.  probs, u and counts may each be host or device
   memory (the runtime tells which).  Integer sums throughout: the counts do not depend on the launch shape. */
int aqc_multinomial_counts(const double* probs, int njobs, int K, int nshots, uint64_t seed, uint64_t run,
                           const double* u, int64_t* counts);
/* counts[pair][9][4] -> out_rdms[pair][4][4]: f = counts / (the setting's total; zero: AQC_ERR_ARG),
   linear inversion rho = 1/4 sum T[P][Q] P (x) Q (T[I][I] = 1; T of two letters from their setting;
   T[P][I], T[I][Q] the signed marginal averaged over the three settings measuring it), then the
   positive-semidefinite rescaling of Smolin, Gambetta and Smith (PRL 108, 070502: eigenvalues in
   descending order, a = 0, i = 4; while mu_i + a / i < 0: a += mu_i, mu_i = 0, i -= 1; lambda_j =
   mu_j + a / i for j <= i) and division by the trace. */
int aqc_tomo_fit(const int64_t* counts, int npairs, double* out_rdms, int on_device);

/* move_all_qubits_to_sorted_ordering (done implicitly by every measurement below). */
int aqc_mps_sort(aqc_mps_t h);
int aqc_mps_sort_batch(aqc_mps_t* hs, int nstates);
/* mps_dot(psi, zero_mps) = <psi|0...0> (aer_mps_backend.py:49-57).  The states' error flags are
   read with the result (AQC_ERR_STATE as aqc_mps_check_batch: work queued by the async applies). */
int aqc_mps_overlap_zero(aqc_mps_t h, double* re, double* im);
int aqc_mps_overlap_zero_batch(aqc_mps_t* hs, int nstates, double* out /* 2*nstates */);
/* mps_dot(a, b) = <a|b>, conjugating a. */
int aqc_mps_dot(aqc_mps_t a, aqc_mps_t b, double* re, double* im);
/* mps_expectation(psi, "Z", i) for all i (aer_mps_backend.py:80-86), out[n]. */
int aqc_mps_z_all(aqc_mps_t h, double* out);
/* extract_amplitude(psi, 2**i) for all i (aer_mps_backend.py:88-93), out[2n]. */
int aqc_mps_amps_hw1(aqc_mps_t h, double* out);
/* Batched forms for many states of the same n (and, for z_all, the same capacity): one set of
   launches for every state -- the softened global cost (aer_mps_backend.py:58-70) and the local cost
   (:72-74, 80-86) of a Rotoselect gate's candidates (cost_minimiser.py:318-368).  out: nstates x n
   doubles (<Z_i>) or nstates x 2n (complex amplitudes).  z_all_batch contracts the left / right
   environments as matrix products (the ISL RDM machinery) instead of aqc_mps_z_all's per-site
   chains; both are full contractions (no canonical form assumed). */
int aqc_mps_z_all_batch(aqc_mps_t* hs, int nstates, double* out);
int aqc_mps_amps_hw1_batch(aqc_mps_t* hs, int nstates, double* out);
/* out[s] = sum_i <Z_i> of hs[s] (sorted first, as z_all_batch) -- the local cost
   0.5 (1 - mean <Z_i>) (aer_mps_backend.py:72-74, 80-86) needs only the sum.  A state copied from
   `base` (aqc_mps_copy / aqc_mps_copy_batch) while base has not changed since contracts only the
   sites it rewrote, against environment pairs of the operator sum_i Z_i cached on base (extended
   as base changes: the Rotoselect prefix of cost_minimiser.py:318-368); any other state takes the
   full chains of z_all_batch.  base itself is not modified and must not be among hs. */
int aqc_mps_z_sum_batch(aqc_mps_t base, aqc_mps_t* hs, int nstates, double* out);
/* <psi|0..0> (out_ov: 2 doubles per state, as aqc_mps_overlap_zero_batch) and, when out_amps is not
   null, <e_i|psi> (2 n doubles per state, as aqc_mps_amps_hw1_batch) -- the global and softened
   costs (aer_mps_backend.py:49-70, 88-93) of a Rotoselect gate's candidates: a state copied from
   `base` while base has not changed since contracts only the sites it rewrote, against zero and
   Hamming-weight-1 rows cached on base; any other state takes the full chains.  base is not
   modified and must not be among hs.  The states' and base's error flags are read with the
   results (as aqc_mps_check_batch would: AQC_ERR_STATE on a capacity overflow of queued work). */
int aqc_mps_zero_hw1_batch(aqc_mps_t base, aqc_mps_t* hs, int nstates, double* out_ov, double* out_amps);

/* ---- candidate sweep: replaces gradients.py:23-124 ------------------------------ */
/* For every pair (pairs[2p], pairs[2p+1]) = (control, target):
 *   g_p = sqrt( sum_k degs[k] * ( -Im( <s|G_k|psi> <psi|U0^dag|s> ) )^2 )
 * |s> is the product state with per-qubit 2-vectors svec[n][2] (complex); u0 and gens are
 * 4x4 (little-endian over (control, target)) matrices of U0 and G_k (NOT their inverses).
 * out: npairs doubles; out_is_device != 0 means `out` is a device pointer (for RCCL).
 * With a host `out` the call returns when the scores are there; with a device `out` it returns
 * once the work is queued on the library's stream: aqc_stream_join orders another stream (the
 * caller's, e.g. the all-gather's) after it, and aqc_stream_wait (called before) orders the sweep
 * after the caller's earlier work on `out`. */
int aqc_pair_grads(aqc_mps_t psi, const double* svec, const int* pairs, int npairs,
                   const double* u0, const double* gens, const double* degs, int ngen,
                   double* out, int out_is_device);
int aqc_pair_grads_batch(aqc_mps_t* psis, int nstates, const double* svec, const int* pairs,
                         int npairs, const double* u0, const double* gens, const double* degs,
                         int ngen, double* out /* nstates*npairs */, int out_is_device);
/* Orders `stream` (a hipStream_t of the current device; NULL = the legacy default stream) after
   everything queued so far on the library's stream of that device, without a host wait. */
int aqc_stream_join(void* stream);
/* The reverse order: the library's stream of the current device waits for everything queued so far
 * on `stream`, without a host wait.  A device-output sweep (out_is_device) is ordered both ways by
 * calling aqc_stream_wait(caller) before it -- so the sweep's writes to `out` follow the caller's
 * earlier kernels on that buffer (a fill, the previous step's reads) -- and aqc_stream_join(caller)
 * after it, so the caller's later kernels see the scores. */
int aqc_stream_wait(void* stream);
/* Best product-state (chi = 1) approximation of psi: the starting circuit
 * starting_circuit="tenpy_product_state" (approximate_compiler.py:222-242, which compresses with
 * tenpy's variational method: trunc_params chi_max = 1, min_sweeps 10, max_sweeps 50).  Alternating
 * two-site updates maximise |<s|psi>| (each pair's optimum is the top singular pair of its 2 x 2
 * environment tensor); a sweep is a left-to-right and a right-to-left pass; the fit stops after
 * min_sweeps once a sweep changes the fidelity by <= tol (relative), or after max_sweeps.
 * svec: n x 2 complex per-qubit vectors (in: initial guess unless guess_from_gamma != 0, which
 * starts from the chi = 1 truncation of the canonical form; out: the fit).  fidelity = |<s|psi>|^2
 * (psi normalised). */
int aqc_mps_product_fit(aqc_mps_t psi, double* svec, int guess_from_gamma, int min_sweeps, int max_sweeps,
                        double tol, double* fidelity, int* sweeps);
/* np.argmax(scores * priorities) with lowest-index tie-break (adapt_compiler.py:832-837).  Device
 * scores are read on the library's stream: order it after their producer (aqc_stream_wait). */
int aqc_argmax_scaled(const double* scores, const double* prio, int count, int scores_is_device,
                      int* best);
/* The same rule for each of nrows score rows at once (row r at scores + r * ld), all pointers on the
 * device, queued on the library's stream without a host wait (order it with aqc_stream_wait /
 * aqc_stream_join): out[r] = row r's arg-max index (as a double), out[nrows + r] = its scaled score
 * -- the per-state selection of a batch of sweeps, laid out for one all-gather. */
int aqc_argmax_scaled_batch(const double* scores, int ld, const double* prio, int count, int nrows,
                            double* out);

/* Diagnostics, lab switches and test hooks (path selection, phase ticks, path counters, a CU-holding
   test load, the SVD kernel on its own) are declared in aqc_hip_diag.h: they are not part of the
   drop-in boundary. */

/* ---- multi-GPU exchange over RCCL ---------------------------------------------
 * The candidate sweep shards the coupling-map pairs across ranks (one process per GPU); its one
 * exchange is an all-gather of the per-pair scores, after which every rank takes the same arg-max
 * (adapt_compiler.py:832-856 -- the reference has no collective: it runs on one host).  For
 * callers without torch.distributed.  aqc_comm_unique_id on one rank, its 128 bytes passed to
 * every rank by the caller's own channel, then aqc_comm_init(id, rank, world) on every rank
 * (collective; the current device, see aqc_init).  Collectives run on the library's stream:
 * aqc_allgather_f64 takes device buffers (send: count doubles, recv: world x count, rank order)
 * and returns once queued, ordered after the library's earlier work (a device-output sweep);
 * aqc_allgather_f64_host / aqc_allreduce_max_f64 take host memory and return complete. */
int aqc_comm_unique_id(char* out /* 128 bytes */);
int aqc_comm_init(const char* unique_id, int rank, int world, aqc_comm_t* out);
int aqc_comm_destroy(aqc_comm_t c);
int aqc_comm_rank(aqc_comm_t c, int* rank, int* world);
int aqc_allgather_f64(aqc_comm_t c, const double* send, double* recv, size_t count);
int aqc_allgather_f64_host(aqc_comm_t c, const double* send, double* recv, size_t count);
int aqc_allreduce_max_f64(aqc_comm_t c, double* value);

#ifdef __cplusplus
}
#endif
#endif /* AQC_HIP_H */
