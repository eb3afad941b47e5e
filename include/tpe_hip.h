/*
 * tpe_hip.h — C-ABI of the MI355X TPE suggest engine (libtpe_hip.so).
 *
 * This boundary replaces the numpy operators that gsmafra/hyperopt evaluates
 * through its pyll interpreter on every tpe.suggest call (reference file:line
 * below).  Plain C types only: device pointers, sizes, an opaque hipStream_t.
 * No allocation, no host synchronisation and no C++ exception crosses it; every
 * entry point returns 0 on success or a negative TPE_E* code, and
 * tpe_last_error() gives a thread-local message.
 *
 * One tpe_run_batch() call evaluates a *batch of problems*.  A problem is one
 * (new_id, hyperparameter) pair of one tree level — the unit the reference
 * handles per parameter in build_posterior (tpe.py:663-701):
 *
 *   sample  C candidates from the "below" Parzen mixture     GMM1 / LGMM1 (tpe.py:62-93, 216-250),
 *                                                           categorical (pyll/stochastic.py:104-142)
 *   score   l(x) = lpdf_below(x),  g(x) = lpdf_above(x)      GMM1_lpdf (tpe.py:104-166),
 *                                                           LGMM1_lpdf (tpe.py:259-301),
 *                                                           categorical_lpdf (tpe.py:50-57)
 *   select  argmax_x  l(x) - g(x), first index on ties      broadcast_best (tpe.py:749-759)
 *
 * The Parzen fit (adaptive_parzen_normal, tpe.py:398-475) and the below/above
 * split (ap_filter_trials, tpe.py:613-641) are done by the caller, which
 * uploads the fitted mixtures as the component tables described below — or,
 * for large continuous above mixtures, left to the device: tpe_fit_above()
 * fits them from device-resident observation columns (see tpe_fit_job).
 */
#ifndef TPE_HIP_H
#define TPE_HIP_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define TPE_ABI_VERSION 24

/* finalize slots per candidate tile: tile_best holds n_tiles * TPE_BEST_PER_TILE entries */
#define TPE_BEST_PER_TILE 8

/* categorical problems with at most this many categories are scored by the
 * sample stage itself (device-drawn candidates) */
#define TPE_SAMPLE_LDS_ROWS 1024
/* cell rows a table workgroup computes (one per wave); a lattice value takes
 * a whole workgroup.  A short side (at most 64 component rows + wide rows,
 * rows_n >= 0) is summed directly, several rows a wave: 5 for a log-polynomial
 * job, 4 for a moment-cell job.  tpe_batch.tab_blocks = sum over such
 * log-polynomial jobs of ceil(n / (5 TPE_TAB_PER_BLOCK)) + over such moment
 * jobs of ceil(n / (4 TPE_TAB_PER_BLOCK)) + over the other cell jobs of
 * ceil(n / TPE_TAB_PER_BLOCK) + over lattice jobs of n (a TPE_F_FGT label's
 * above cells: none, the box stage builds them) */
#define TPE_TAB_PER_BLOCK 8
/* 16-B units of one cell row of a TPE_TAB_CELLS table */
#define TPE_TAB_ROW_UNITS 3

/* problem families: {Gaussian, log-Gaussian} x {continuous, quantized} + categorical */
enum {
  TPE_FAM_GAUSS = 0,       /* GMM1_lpdf, q=None   (uniform, normal)            */
  TPE_FAM_LOGGAUSS = 1,    /* LGMM1_lpdf, q=None  (loguniform, lognormal)      */
  TPE_FAM_QGAUSS = 2,      /* GMM1_lpdf, q        (quniform, qnormal)          */
  TPE_FAM_QLOGGAUSS = 3,   /* LGMM1_lpdf, q       (qloguniform, qlognormal)    */
  TPE_FAM_CATEGORICAL = 4  /* categorical_lpdf    (randint, choice, pchoice)   */
};

/* problem flags */
enum {
  TPE_F_HAS_LOW = 1,   /* low bound present (reference: low is not None)   */
  TPE_F_HAS_HIGH = 2,  /* high bound present                                */
  TPE_F_POOLED = 4,    /* candidates pooled with the other ids of the label (see "Pooled labels") */
  TPE_F_CAT_LAZY = 8,  /* categorical, <= 64 categories, best-scoring drawable category with selection
                          probability >= 2^-16: device-drawn batches without per-candidate outputs
                          score it in the select stage by scanning draws in index order until no
                          undrawn category can still win (usually one 1024-draw chunk) */
  TPE_F_NO_TABLE = 16, /* tpe_label_in: score this label per candidate (no lattice table), e.g. when
                          the caller supplies candidates that need not lie on the quantization lattice */
  TPE_F_PREFIT = 32,   /* tpe_tree_label: fit this label up front on the host worker threads (the
                          caller's hint: the labels its previous suggest on the space used); no label
                          flagged: every natively fitted label with enough observations */
  TPE_F_FGT = 64,      /* tpe_problem (set by the packer): a device-fitted TPE_TAB_CELLS label whose
                          above cells are built from Hermite box moments (see "Box moments") */
  TPE_F_REMOTE = 128,  /* tpe_tree_label: another rank evaluates this label (hyperparameter-axis
                          shard, see "Shard axes"): it is neither fitted nor run here; its values
                          are NaN and its activity is the tree's.  Not allowed on a gate. */
  TPE_F_LOGPOLY = 256  /* tpe_problem (set by the packer): a TPE_TAB_CELLS label whose table holds
                          log-polynomial rows of both sides on one cell grid (see "Tabulated
                          scoring"; its two table jobs have kind TPE_TAB_LOGPOLY) */
};

/* box moments (see "Box moments" below): Hermite terms per box, 16-B units per box record */
#define TPE_FGT_P 16
#define TPE_FGT_BOX_UNITS 9

/* tabulated scoring of a problem (tpe_problem.tab_mode, see "Tabulated scoring") */
enum {
  TPE_TAB_NONE = 0,     /* scored by the above / finalize stages (per candidate)                  */
  TPE_TAB_CELLS = 1,    /* continuous f32: per-cell Taylor moment tables of both mixtures          */
  TPE_TAB_LATTICE = 2,  /* quantized: exact {l, g} per lattice value of the candidate range        */
  TPE_TAB_LOGPOLY = 3   /* tpe_tab_job kind of a TPE_F_LOGPOLY label's sides (problems keep
                           TPE_TAB_CELLS)                                                         */
};

/* tpe_batch.flags / tpe_level_run flags */
enum {
  TPE_BATCH_NO_EXPAND = 1,  /* pruned f32 kernel: evaluate every component exactly (no local expansion) */
  TPE_BATCH_WRITE_CAND = 2, /* store every drawn candidate value in cand (else only where a later stage
                               reads it: quantized families and TPE_PREC_F64; the winner's value is
                               re-drawn by the select stage) */
  TPE_BATCH_NO_FUSE = 4,    /* score every continuous tile in the finalize stage (no fused finalize
                               in the above kernel) */
  TPE_BATCH_ORDERED_DRAWS = 8, /* sorted problems draw ordered candidates, no sort (else i.i.d.
                                  draws + sort) — see "Ordered draws" below */
  TPE_BATCH_TAB_EXACT = 16,    /* test hook: flag every table cell, so every candidate of a
                                  TPE_TAB_CELLS problem takes the exact-sum fallback */
  TPE_BATCH_NO_TAB_FAST = 32, /* tpe_level_run: the general sample-stage kernel even where the
                                  specialised one applies (tpe_batch.tab_fast; A/B, tests) */
  TPE_BATCH_NO_FAST2 = 64      /* tpe_level_run: k_sample_tab's 1024-thread FAST pass where
                                  k_sample_fast applies (tab_fast = 1 for log-polynomial levels; tests) */
};

/* precision of the continuous (non-quantized) families; quantized families
 * always evaluate the mixture mass in float64 (cancellation of Phi(ub)-Phi(lb)) */
enum { TPE_PREC_F32 = 0, TPE_PREC_F64 = 1 };

/* error codes */
enum { TPE_OK = 0, TPE_E_ARG = -1, TPE_E_HIP = -2, TPE_E_NODEV = -3, TPE_E_SPACE = -4 };

/*
 * One problem (256 bytes).  Component tables (device, caller-owned):
 *   comp32[k] = float4 {mu_hi, mu_lo, a, c}      families 0/1 at TPE_PREC_F32
 *   comp64[k] = double4 {mu, a, c, 0}            families 0/1 at TPE_PREC_F64
 *   comp64[k] = double4 {mu, b, w, 0}            families 2/3 (b = max(sqrt2*sigma, EPS))
 *   comp64[k] = double4 {log p_k, p_k, 0, 0}     family 4
 * For families 0/1 the mixture log-density is
 *   lpdf(x) = ln2 * log2( sum_k 2^(c_k - (a_k * (t - mu_k))^2) ) + base  [- ln x for LOGGAUSS]
 * with t = x (GAUSS) or ln x (LOGGAUSS); the host folds weights, 1/Z,
 * p_accept and a per-mixture shift (max_k c_k = 0) into c_k and base.
 * Families 2/3:  lpdf(x) = ln( sum_k w_k Phi(zu_k) - w_k Phi(zl_k) ) + base.
 *
 * Pruned above mixture (families 0/1, f32): the above components are sorted by
 * mu; the `wide_len` widest (incl. the prior) are copied to comp32[wide_off..]
 * and set to c = -inf in the sorted list.  A wave of sorted candidates spanning
 * [tmin, tmax] evaluates every wide component plus the sorted components with
 * mu in [tmin - R, tmax + R], R = sqrt(narrow_cmax - lb + 45) / narrow_amin,
 * lb = prior_c - (prior_a * max|t - prior_mu|)^2 a lower bound of log2 s(t):
 * every skipped term is < 2^-45 of the sum.  grid[grid_off .. +grid_n] maps
 * value buckets (grid_lo + g / grid_inv) to the first sorted component with
 * mu >= the bucket edge (grid_inv = 0, every f32 mean equal: bucket 0 is
 * component 0 and every later bucket the component count, so a window of
 * buckets holds every component).  narrow_amin <= 0 disables pruning.  With pruning,
 * work item `split` of a tile evaluates the split-th of its n_splits equal
 * parts of each wave's window (k_start/k_end are ignored).
 *
 * Sorted problems (sort_slot >= 0, the pruned ones) own the candidate range
 * [0, sort_count) of the batch; the sort key is sort_slot << key_bits | value
 * bucket.  Other problems' candidates follow and are never sorted.
 *
 * Pooled labels (a pruned label active for several ids of the level — batched
 * suggest): its problems share the mixtures, so their candidates are sorted as ONE
 * population (one sort slot, key bits sized for n_ids x n_cand) and every wave
 * spans a narrow range however small n_cand is.  A sorted position may then hold
 * any of the label's problems' candidates: the scoring stages fold each candidate
 * into its own problem's pool_best[problem] (atomicMax of a u64 key: the f64 score
 * mapped to an order-preserving integer, its low bits replaced by the
 * complemented candidate index — np.argmax order at ~2^-40 relative score
 * resolution), and k_select re-evaluates the winner's l and g exactly.
 *
 * Ordered draws (TPE_BATCH_ORDERED_DRAWS; device-drawn sorted problems at
 * TPE_PREC_F32): instead of C i.i.d. draws that are then sorted, the
 * sample stage draws the C order statistics of C uniforms,
 * U_g = (E_0 + .. + E_g) / (E_0 + .. + E_Cg), E_i = -ln u_i (Philox counter =
 * global index i), and maps each through the mixture: component k with
 * cum_{k-1} <= U_g < cum_k, then the component's truncated-normal inverse CDF at
 * (U_g - cum_{k-1}) / (cum_k - cum_{k-1}).  The multiset of candidates has the
 * law of C i.i.d. mixture draws (so does its argmax); candidates come out sorted
 * within each component, which is all the pruned kernel needs.  The prefix sums
 * use fixed 64-index blocks of the GLOBAL index (draw_pref: per sorted problem,
 * draw_blocks exclusive block prefixes + the total), so every shard count draws
 * the same values bit for bit.
 *
 * Tabulated scoring (tab_mode != TPE_TAB_NONE): the score of a candidate is a
 * function of its value alone, so each hyperparameter's l and g are tabulated
 * once per level — shared by every new_id of the label — and the sample stage
 * scores each draw from the tables (no candidate stores, no sort, no above or
 * finalize work):
 *   TPE_TAB_CELLS (families 0/1, f32): side s (0 below, 1 above) splits
 *     [tab_lo[s], tab_lo[s] + tab_n[s] / tab_inv[s]) into tab_n[s] cells of
 *     half-width h with a_max * h <= 0.05 (a_max: the narrowest component).
 *     About its centre c a component's term is 2^v exp(B u + G u^2),
 *     u = (t - c) / h, |G| <= 0.0017; a cell row holds the degree-10 Taylor
 *     moments of the sum of the terms within 2^-50 of its largest one
 *     (|B| <= 0.6, truncation < 4e-8 relative) — a 48-B row of floats
 *     {M0..M10, m (log2 shift)}: log2 s(t) = m + log2(sum_n M_n u^n).  Cell j's
 *     centre and half-width are c = fma(j + 0.5, w, tab_lo), h = w / 2 with
 *     w = 1 / tab_inv, all in f32 (the table and the sample stages compute them
 *     alike).  m = NaN (a significant term too narrow to expand) and t outside
 *     the cells fall back to the exact sum.
 *     TPE_F_LOGPOLY (both sides fit the sample stage's LDS on one grid: the
 *     finer side's cells for both): one table of 48-B rows, row j = {b_0, a_0,
 *     b_1, a_1, .., b_5, a_5} (the sides interleaved: one packed Horner chain
 *     evaluates both): the degree-5 polynomials in u of log2 s_below(t) and log2
 *     s_above(t) (shift included) on cell j — the table stage evaluates each
 *     side's moment series in f64 at the 6 Chebyshev nodes of [-1, 1],
 *     interpolates, and checks the polynomial at u = 0, +-1/2, +-1 against the
 *     series (|error| <= 1e-7 (1 + |log2 s|)); a side that fails, or whose
 *     cell is flagged, gets b_0 (a_0) = NaN and its candidates the exact sum.
 *     One row, two degree-5 Horner sums and no log2 per candidate instead of
 *     two rows, two degree-10 sums and two log2.
 *   TPE_TAB_LATTICE (families 2/3): every candidate is x = m q (np.round,
 *     tpe.py:90-93, 248-249); row m - lat_lo of the table (tab_n[0] rows of
 *     double2 {l, g}, float64, reference operation order per component) holds
 *     its scores; other values (injected candidates) are scored directly.
 *     ABI 20: the rows are followed by tab_n[0] + 1 float entry thresholds
 *     (ceil((tab_n[0] + 1) / 4) units): thr[m] = the smallest f32 coordinate t
 *     in the clip range whose np.round(x / q) >= lat_lo + m (+inf: none), so a
 *     device draw t takes row #{m : thr[m] <= t} - 1 with no f64 arithmetic
 *     (k_sample_fast; k_sample_tab quantises directly, with the same result).
 * Tables live in `tab` (16-B units; tab_off[s] = first unit) and are built by
 * the table stage from the problem's component rows (after the device fit).
 *
 * Box moments (TPE_F_FGT: device-fitted above mixtures of a TPE_TAB_CELLS
 * label).  adaptive_parzen_normal clips every bandwidth to >= prior_sigma /
 * min(100, 1 + K) (tpe.py:465-470), so a large history's above components
 * share that narrowest sigma (a = fgt_a in the rows) almost everywhere: their
 * sum is a Gauss transform with one width d = 1 / (fgt_a sqrt(ln 2)).  The
 * box stage (k_boxes) cuts [fgt_lo, fgt_lo + fgt_n d) into boxes of width d
 * and gives each box its Hermite moments A_n = sum_k 2^c_k y_k^n / n!
 * (y_k = (mu_k - centre) / d, n < TPE_FGT_P, f64, fixed-order reductions);
 * a cell then gets its Taylor moments from the boxes within reach,
 * B_m = (-1)^m / m! sum_b sum_n A_bn h_(n+m)(x_b) (h_j(x) = e^-x^2 H_j(x),
 * x_b = (centre_cell - centre_b) / d) — about 16 boxes per cell instead of
 * every component within reach — plus the components of other widths (the
 * wide list, and any "odd" component a box counts) summed directly.  A cell
 * whose truncation bound (Cramer: sum_b 1.09 W_b e^(-x_b^2 / 2) eps_P) is not
 * below 2^-25 of its sum, and every cell of a label whose components do not
 * all lie in the boxes, is built by the direct path instead.  Box records
 * follow the label's above cells in `tab` at fgt_off: one header unit {int32
 * ok, ...} and TPE_FGT_BOX_UNITS units per box {double A[TPE_FGT_P]; int32
 * k_lo, k_hi, n_odd, 0}.
 *
 * samp[k] = double[8] {cum, mu, sigma, fa, fb, flip, 0, 0}: below-mixture
 * sampler table; cum = selection CDF (∝ w_k * mass_k when bounded); fa, fb =
 * Phi of the (mirrored if flip) standardised truncation bounds; family 4 uses cum.
 */
typedef struct tpe_problem {
  int32_t family, flags;
  int32_t n_cand;        /* candidates of this problem on this device          */
  int32_t n_upper;       /* categorical: number of categories                  */
  int64_t cand_off;      /* element offset into cand / coord / keys / l_out    */
  int64_t cand_base;     /* global index of local candidate 0 (shards, RNG)    */
  int64_t n_cand_global; /* candidates of the problem over all shards (= n_cand unsharded) */
  int32_t n_splits;      /* splits of the bulk tiles (tiles carry their own)   */
  int32_t tile_off;      /* first candidate tile of this problem               */
  int32_t n_tiles;       /* candidate tiles of this problem                    */
  int32_t samp_off;
  int32_t samp_len;
  int32_t below_off;
  int32_t below_len;
  int32_t above_off;
  int32_t above_len;
  int32_t wide_off;      /* always-evaluated wide components (pruned mode)     */
  int32_t wide_len;
  int32_t grid_off;
  int32_t grid_n;
  int32_t sort_slot;     /* rank among the batch's sorted problems, -1: unsorted */
  double low, high, q;   /* bounds in sampling space (log space for LGMM1)     */
  double below_base;     /* additive constant of the below lpdf                */
  double above_base;     /* additive constant of the above lpdf                */
  float prior_mu, prior_a, prior_c, narrow_cmax;
  float narrow_amin, grid_lo, grid_inv;
  float key_lo, key_inv; /* sort-key bucket of t: floor((t - key_lo) * key_inv)  */
  int32_t pool_first;    /* pooled: the label's first problem (else -1)         */
  uint32_t key0, key1;   /* Philox-4x32-10 key (suggest seed)                  */
  uint32_t ctr2, ctr3;   /* Philox counter high words (label index, new id)    */
  int32_t tab_mode;      /* TPE_TAB_*                                          */
  int32_t tab_off[2];    /* first 16-B unit of the below / above table in `tab` (lattice: [0]) */
  int32_t tab_n[2];      /* cells per side (lattice: tab_n[0] = lattice values) */
  float tab_lo[2], tab_inv[2];  /* cell j of side s: [tab_lo[s] + j / tab_inv[s], + 1 / tab_inv[s]) */
  float fgt_a;           /* TPE_F_FGT: a of the narrowest (sigma-clipped) components  */
  int64_t lat_lo;        /* lattice: index m of table row 0 (value lat_lo * q) */
  int32_t fgt_off;       /* TPE_F_FGT: first 16-B unit of the box records in `tab`    */
  int32_t fgt_n;         /* TPE_F_FGT: boxes of width 1/(fgt_a sqrt(ln 2)) from fgt_lo */
  double fgt_lo;
} tpe_problem;

/* one table of the table stage: a side of a TPE_TAB_CELLS label (4 cells per
 * 256-thread block) or a TPE_TAB_LATTICE label (1 lattice value per block).
 * `problem` is the label's first problem row (its mixtures are the label's). */
typedef struct tpe_tab_job {
  int32_t problem;
  int32_t side;          /* cells: 0 below, 1 above                             */
  int32_t kind;          /* TPE_TAB_CELLS | TPE_TAB_LATTICE                     */
  int32_t n;             /* cells / lattice values                              */
  int32_t off;           /* first 16-B unit of the table                        */
  int32_t block0;        /* first block of this job in the table stage's grid   */
  /* cells: the side's component rows (comp32 [rows_off, rows_off + rows_n) then
   * [wide_off, wide_off + wide_n)) and cell geometry (the problem's tab_lo /
   * tab_inv of this side), so the table stage reads no problem row; rows_n < 0:
   * read them from the problem (a device-fitted above side: the fit writes them) */
  int32_t rows_off, rows_n, wide_off, wide_n;
  float lo, inv;
} tpe_tab_job;

/* candidate tile: 2048 consecutive candidates of one problem; its above-mixture
 * partial sums are rows work_first .. work_first + n_splits - 1 of `part` */
typedef struct tpe_tile {
  int32_t problem;
  int32_t cand_start;
  int32_t work_first;    /* first work item (= part row) of this tile          */
  int32_t n_splits;      /* its work items (0: no above stage)                 */
} tpe_tile;

/* above-mixture work item: one candidate tile x one component range; writes
 * the tile's partial sums to part[row * 2048 .. + 2048), row = its index in
 * the batch's work list */
typedef struct tpe_work {
  int32_t problem;
  int32_t split;
  int32_t cand_start;
  int32_t k_start;
  int32_t k_end;
  int32_t n_splits;      /* work items of this tile                            */
} tpe_work;

/* best of one finalize slot (TPE_BEST_PER_TILE per tile), written by the finalize stage */
typedef struct tpe_best {
  double score, l, g;
  int64_t idx;           /* local candidate index, -1 if none */
} tpe_best;

/* per-problem result */
typedef struct tpe_result {
  double score, l, g;
  double value;          /* the chosen candidate                               */
  int64_t idx;           /* local candidate index, -1 if the problem is empty  */
  int64_t global_idx;    /* cand_base + idx                                     */
} tpe_result;

/*
 * Device Parzen fit of one continuous above mixture (families 0/1, f32 tables):
 * adaptive_parzen_normal (tpe.py:398-475) of the label's observations that are
 * not in the below set (ap_filter_trials, tpe.py:613-641), written straight
 * into the pruned comp32 layout above.
 *
 * Device value order.  The reference argsorts the above observations on every
 * suggest (tpe.py:427).  Here each device-fitted label keeps a RESIDENT value
 * order of ALL its observations in HBM — (t, i) pairs sorted by t ascending,
 * NaN last, ties by i (t = x, or ln x for LOGGAUSS; i = position in tid
 * order) — owned by the caller and extended, not rebuilt: the history is
 * append-only, so a suggest only merges the observations appended since the
 * order was last written (obs[n_ord_in .. n_obs)).  Stages (tpe_fit_above):
 *   chunks   the new observations, 8192 at a time, sorted in LDS (bitonic)
 *   passes   merge-path merges of the sorted chunks (only when a job has more
 *            than 8192 new observations, i.e. the first suggest)
 *   merge    merge-path merge of the resident order ord_*_in [n_ord_in] with the
 *            sorted new batch into ord_*_out [n_obs] (skipped when nothing is new:
 *            the order is then read from ord_*_in)
 *   compact  the order without the below observations, each with its rank among
 *            the above observations in tid order (the linear-forgetting weight
 *            index) — exactly the stable argsort of the above observations
 *   build    one workgroup per job: prior insertion (searchsorted left), sigma
 *            from neighbour gaps, clip, LF weights, normalisation, {mu, a, c}
 *            rows, wide list, grid; patches the job's problem rows (above_base,
 *            wide_len, prior_*, narrow_*, grid_lo/inv)
 * No sort of the whole history runs after the first suggest.  DELTA MODE: a job
 * with 1 .. TPE_FIT_DELTA_MAX new observations and ord_*_out NULL is not merged:
 * its new observations are sorted and placed among the resident ones (their
 * ranks), and the build reads the resident order and them as one virtual order
 * — the merge pass over the whole order waits until the new ones outgrow the
 * delta (FMinIter's one observation per suggest: one merge every
 * TPE_FIT_DELTA_MAX suggests); ord_*_in stays the caller's order of the first
 * n_ord_in.  A steady-state suggest costs the build (plus, every
 * TPE_FIT_DELTA_MAX appends, one merge pass over each label's order).
 * The host reserves above_off[0 .. K) + wide_off[0 .. 16) rows and grid_n + 1
 * grid entries (K = n_obs - n_below + 1, grid_n = min(4096, 4K)).
 */
#define TPE_FIT_DELTA_MAX 16
typedef struct tpe_fit_job {
  const double* obs;     /* device: the label's observations in tid order, in the kernel
                            coordinate t (x, or the caller's np.log(x) for LOGGAUSS) */
  int64_t n_obs;
  int64_t seg_off;       /* first slot of this job in the fit scratch buffers (fit_seg)   */
  int32_t below_off;     /* below_idx[below_off ..]: ascending indices into obs */
  int32_t n_below;
  int32_t family, flags, lf;
  int32_t problem_first, n_problems;  /* problem rows this mixture serves      */
  int32_t above_off, wide_off, grid_off, grid_n;
  int32_t reserved;
  double prior_mu, prior_sigma, prior_weight, low, high;
  /* resident value order (device, caller-owned): the first n_ord_in observations
   * sorted, and where the order of all n_obs goes when n_ord_in < n_obs */
  const double* ord_key_in; const uint32_t* ord_idx_in; int64_t n_ord_in;
  double* ord_key_out; uint32_t* ord_idx_out;
} tpe_fit_job;

/* all device pointers of one batch (the struct itself lives in host memory) */
typedef struct tpe_batch {
  const tpe_problem* problems; int32_t n_problems;
  int32_t precision;     /* TPE_PREC_F32 | TPE_PREC_F64                         */
  int32_t sample;        /* 1: draw candidates on device (Philox); 0: caller filled cand/coord */
  int32_t sort_end_bit;  /* keys sorted on bits [0, sort_end_bit); 0 = no sort  */
  int32_t key_bits;      /* value-bucket bits of the sort key (problem << key_bits | bucket) */
  int32_t flags;         /* TPE_BATCH_* options (0 = defaults)                  */
  const float* comp32;   /* [n][4]                                             */
  const double* comp64;  /* [n][4]                                             */
  const double* samp;    /* [n][8]                                             */
  const int32_t* grid;   /* pruning grids                                      */
  double* cand;          /* [total_cand] candidate values (see TPE_BATCH_WRITE_CAND) */
  float* coord;          /* [total_cand] kernel coordinate t in f32 (x or ln x) */
  uint32_t* keys;        /* [total_cand] (problem << key_bits | value bucket of t) */
  uint64_t* vals;        /* [total_cand] (position << 32) | f32 bits of t       */
  uint32_t* keys_sorted; /* [total_cand] (== keys when not sorting)            */
  uint64_t* vals_sorted; /* [total_cand] (== vals when not sorting)            */
  void* sort_tmp; uint64_t sort_tmp_bytes;   /* tpe_sort_workspace_bytes()     */
  int64_t total_cand;
  const tpe_tile* tiles; int32_t n_tiles; int32_t n_fin_tiles;
  int64_t sort_count;    /* candidates [0, sort_count) are sorted (sorted problems first) */
  const int32_t* fin_tiles; /* [n_fin_tiles] tiles the finalize stage scores when the candidates
                               are device-drawn (the others are scored by the sample stage —
                               categorical — or the fused above stage — one-split continuous
                               f32);
                               NULL: every tile */
  /* above-mixture work list, ordered [continuous | quantized Gauss | quantized log] */
  const tpe_work* work;
  int32_t n_work_cont, n_work_qgauss, n_work_qlog;
  int32_t fgt_max_boxes; /* most boxes of a TPE_F_FGT problem (0: none; the box stage's grid) */
  double* part;          /* above-mixture partial sums: [n_work][2048]          */
  double* l_out;         /* optional [total_cand] (original order); NULL to skip */
  double* g_out;         /* optional [total_cand]; NULL to skip                 */
  tpe_best* tile_best;   /* [n_tiles * TPE_BEST_PER_TILE]                      */
  tpe_result* result;    /* [n_problems]                                       */
  unsigned long long* ce_count; /* optional [2 * n_work_cont]: per work item of the pruned
                                   kernel, {exactly evaluated component x candidate pairs,
                                   components summed by the local expansion}; NULL to skip */
  /* device Parzen fits (n_fit == 0: none); they patch rows of `problems` */
  const tpe_fit_job* fit; int32_t n_fit;
  int32_t fgt_max_cells; /* most above cells of a TPE_F_FGT problem (built by the box stage) */
  const int32_t* below_idx;   /* below indices of every job                        */
  const int64_t* fit_seg;     /* [n_fit + 1] segment offsets into the fit scratch: a job's
                                 segment holds max(n_obs - n_below, n_obs - n_ord_in, n_below,
                                 64 + 2 * TPE_FIT_DELTA_MAX [+ 2304 per 2048 components of a
                                 delta-mode job]) */
  int64_t fit_total;          /* fit_seg[n_fit]                                    */
  double* fit_keys; double* fit_keys_sorted;        /* [fit_total] scratch (ping-pong) */
  uint32_t* fit_vals; uint32_t* fit_vals_sorted;    /* [fit_total]                */
  int64_t fit_max_new;        /* most new observations of one job (n_obs - n_ord_in) */
  int64_t fit_max_obs;        /* most observations of one job                       */
  int64_t fit_max_merge;      /* most new observations of a job that merges them (0: none) */
  int64_t fit_n_delta;        /* jobs in delta mode (new observations, no ord_*_out) */
  /* ordered draws: [n_sorted][draw_blocks + 1] doubles, draw_blocks = ceil((C_global + 1) / 64) */
  double* draw_pref; int64_t draw_blocks; int32_t n_sorted;
  int32_t tab_fast;      /* >= 1: the candidates are device-drawn at TPE_PREC_F32, early selection is on,
                            nothing per candidate is written and every tabulated problem has
                            1..TPE_SAMPLE_LDS_ROWS sampler rows: the sample stage's specialised kernels —
                            1 + U (ABI 20; every tabulated problem a TPE_F_LOGPOLY cells table of <= 896
                            rows or a lattice of <= 1024 values, <= 64 sampler rows): k_sample_fast in
                            512-thread workgroups taking U 16-B units of LDS (3 per cell row; a lattice
                            value's {l, g} unit plus its 4-B score rank), three a CU; 1: every tabulated
                            problem a TPE_F_LOGPOLY cells table of <= 2048 rows, in 1024-thread
                            workgroups (tpe_level_run sets it; 0: the general kernel) */
  unsigned long long* pool_best;   /* [n_problems] (pooled problems; see "Pooled labels") */
  /* tabulated scoring: table jobs and the table storage (16-B units) */
  const tpe_tab_job* tab_jobs; int32_t n_tab_jobs; int32_t tab_blocks;
  void* tab; int64_t tab_units;
  /* sample-stage tile lists (NULL: every tile through the generic sample kernel):
   * samp_tiles[0 .. n_samp_tiles) = the untabulated tiles, lazy categorical ones
   * last (the first n_samp_eager of them skip those when the lazy scan applies);
   * tab_tiles[0 .. n_tab_tiles) = the tabulated tiles (one 2048-candidate block each) */
  const int32_t* samp_tiles; int32_t n_samp_tiles; int32_t n_samp_eager;
  const int32_t* tab_tiles; int32_t n_tab_tiles;
  /* early selection (needs tables, sampled candidates, tab_tiles and
   * run_best): the sample stage writes, for every run of consecutive tiles of
   * one tabulated problem a workgroup processes, the run's best candidate —
   * score, l, g, index and its drawn value — to run_best[first tile of the run]
   * (host-visible memory; the caller reduces a problem's runs with np.argmax
   * semantics: tpe_level_run does); each lazy categorical problem is selected
   * by the table stage; the select stage runs only for the n_late others (not
   * at all when n_late == 0).  0: the select stage selects every problem. */
  int32_t early_select;
  tpe_result* run_best;  /* [n_tiles], device address of host-visible memory */
  int32_t n_late;
  int32_t tiles_per_problem;   /* > 0: every problem has this many tiles, tile t = {t / tiles_per_problem,
                                  (t % tiles_per_problem) * 2048} (the sample stage then reads no
                                  tile descriptors); 0: read them */
} tpe_batch;

/* ABI version (TPE_ABI_VERSION) of the loaded library */
int tpe_abi_version(void);

/* thread-local message of the last failing call on this thread ("" if none) */
const char* tpe_last_error(void);

/* number of visible HIP devices (0 and TPE_E_NODEV when none) */
int tpe_device_count(int* n);

/* candidates per tile (2048) — the caller sizes tiles / work items with it */
int tpe_tile_size(void);

/* device address of page-locked host memory (NULL when the device cannot
 * address it): look it up once per allocation for tpe_level_ws.pinned_dev */
int tpe_pinned_device_address(void* host, void** dev);

/* device workspace (bytes) the candidate sort needs for `total_cand` candidates */
int tpe_sort_workspace_bytes(int64_t total_cand, uint64_t* bytes);

/* fit (when n_fit > 0) -> tables -> sample (optional) -> sort -> score -> select, enqueued on `stream` (hipStream_t);
 * asynchronous: results are valid once the stream reaches this point. */
int tpe_run_batch(const tpe_batch* batch, void* stream);

/* the stages one by one (same semantics; used by tests and the profiler) */
int tpe_fit_above(const tpe_batch* batch, void* stream);  /* device Parzen fits */
int tpe_tables(const tpe_batch* batch, void* stream);     /* score tables of tabulated labels */
int tpe_sample(const tpe_batch* batch, void* stream);     /* draw + sort keys */
int tpe_sort(const tpe_batch* batch, void* stream);
int tpe_score_above(const tpe_batch* batch, void* stream);
int tpe_finalize(const tpe_batch* batch, void* stream);
int tpe_select(const tpe_batch* batch, void* stream);

/* ------------------------------------------------------------------------
 * Native host runtime (tpe_host.cpp): the Parzen fit and the packing of one
 * tree level into the tables above.  Host pointers only.
 * ---------------------------------------------------------------------- */

/* one hyperparameter of a level: its fitted posterior and the new_ids it is
 * active for (mixtures are float64 host arrays; categorical: below_w / above_w
 * are the probabilities, *_k = number of categories).
 * Device-fitted above mixture (families 0/1, TPE_PREC_F32 only): above_w/mu/
 * sigma NULL, dev_obs = the label's device observation column (n_obs kernel
 * coordinates t in tid order: x, or np.log(x) for LOGGAUSS), below_idx = host array of the n_below ascending indices of the
 * below observations in it, above_k = n_obs - n_below + 1; prior_* and lf are
 * the fit parameters; ord_* = the label's resident value order (tpe_fit_job:
 * ord_*_in may be NULL when n_ord_in = 0, ord_*_out may be NULL when
 * n_ord_in = n_obs or, delta mode, when 0 < n_obs - n_ord_in <= TPE_FIT_DELTA_MAX
 * and n_ord_in > 0).  After the level has run, ord_*_out holds the order of
 * all n_obs observations whenever it was given. */
typedef struct tpe_label_in {
  int32_t family, flags, upper, label_ix;
  double low, high, q;
  const double* below_w; const double* below_mu; const double* below_sigma; int64_t below_k;
  const double* above_w; const double* above_mu; const double* above_sigma; int64_t above_k;
  const int64_t* ids; int64_t n_ids;
  const double* dev_obs; int64_t n_obs;
  const int32_t* below_idx; int32_t n_below; int32_t lf;
  double prior_mu, prior_sigma, prior_weight;
  const double* ord_key_in; const uint32_t* ord_idx_in; int64_t n_ord_in;
  double* ord_key_out; uint32_t* ord_idx_out;
} tpe_label_in;

/* where tpe_host_pack_level put each table in the blob (byte offsets).  The
 * device-fitted rows (end of the grid and comp32 sections) are written by
 * tpe_fit_above: only [0, copy_end) and [off_comp32, off_comp32 + copy2_len)
 * need the host -> device copy. */
typedef struct tpe_pack_info {
  int64_t off_problems, off_tiles, off_work, off_comp32, off_comp64, off_samp, off_grid;
  int64_t n_problems, n_tiles;
  int32_t n_work_cont, n_work_qgauss, n_work_qlog, any_pruned;
  int64_t part_total, blob_bytes;
  int32_t key_bits, sort_end_bit;   /* sort-key layout for tpe_batch (sort_end_bit 0: no sort) */
  int64_t off_fit, off_below_idx, off_fit_seg;
  int32_t n_fit, fgt_max_boxes;     /* device fits; most boxes of a TPE_F_FGT label */
  int64_t fit_total;
  int64_t sort_count;               /* candidates of the sorted (pruned) problems */
  int64_t off_fin_tiles, n_fin_tiles;   /* tpe_batch.fin_tiles */
  int64_t fit_max_new;                  /* tpe_batch.fit_max_new */
  int64_t fit_max_obs;                  /* tpe_batch.fit_max_obs */
  int64_t fit_max_merge;                /* tpe_batch.fit_max_merge */
  int64_t fit_n_delta;                  /* tpe_batch.fit_n_delta */
  int64_t n_sorted, draw_blocks;        /* tpe_batch.n_sorted / draw_blocks */
  int64_t n_pooled;                     /* pooled problems (tpe_batch.pool_best needed) */
  int64_t off_tab_jobs, n_tab_jobs, tab_blocks, tab_units;   /* tabulated scoring (tpe_batch.tab_*) */
  int64_t off_samp_tiles, n_samp_tiles, n_samp_eager, off_tab_tiles, n_tab_tiles;   /* tpe_batch tile lists */
  /* expanded level (see "Expanded levels"; n_expand = 0: not expanded): off_expand holds
   * tpe_problem templates[n_expand], then (at the next 256-B boundary) int32 first[n_expand + 1],
   * then (at the next 256-B boundary) uint32 new_id[n_problems]; the problems and tiles sections
   * (and the tabulated tile list, the identity) are device-only */
  int64_t off_expand, n_expand;
  int64_t fgt_max_cells;                /* most above cells of a TPE_F_FGT label (tpe_batch) */
  /* ABI 20: the blob's host-written byte ranges [up_off[i], up_off[i] + up_len[i]), i < n_up
   * (the upload; everything else is device-only: the device-fitted rows and grid, the fit
   * patches, an expanded level's problems and tiles).  Layout: fit jobs, below positions,
   * fit segments, grid (host | device from a 256-B boundary), comp32 (host | device), fit
   * patches (off_patch: one tpe_problem per problem, the fields the device fit writes,
   * applied to the problem rows after the upload), problems, tiles, comp64, sampler rows,
   * then work, finalize tiles, table jobs, tile lists and the expanded templates. */
  int64_t up_off[4], up_len[4];
  int32_t n_up, pad_;
  int64_t off_patch;                    /* 0: no device fit */
} tpe_pack_info;

/* ------------------------------------------------------------------------
 * Expanded levels.  A batched level (>= 256 problems) whose labels all score
 * from tables (cells or lattice) has problems that differ from their label's
 * only in cand_off (= r * n_cand), ctr3 (the new id) and tile_off (= r *
 * n_tiles), and tiles {r, j * 2048, 0, 0} in order, all of them tabulated.
 * tpe_host_pack_level then writes one problem template per label and the new
 * ids instead of ~270 B per (label, id), and tpe_level_run's device writes the
 * problems and tiles (k_expand) right after the upload: a 20-label x 4096-id
 * level packs and uploads ~0.4 MB of descriptors instead of ~22 MB.
 * ---------------------------------------------------------------------- */

/* adaptive_parzen_normal (tpe.py:398-475) with the caller's sort permutation
 * `order` of obs (np.argsort; may be NULL when n < 2).  Writes n+1 components
 * (w, mu, sigma) sorted by mu; returns the prior's position or a TPE_E* code. */
int64_t tpe_host_fit_parzen(const double* obs, int64_t n, const int64_t* order, double prior_weight,
                            double prior_mu, double prior_sigma, int32_t lf, double* w, double* mu, double* sigma);

/* ap_filter_trials + adaptive_parzen_normal of both sides of one continuous
 * label (tpe.py:613-641, 398-475, 485-568).  x: the label's (transformed)
 * observations, tids strictly ascending; order: a permutation sorting x
 * ascending (the history keeps it incrementally); below_tids ascending.  Each
 * side's permutation is `order` filtered to that side — the permutation
 * np.argsort gives when no value of the side repeats; a side with repeated
 * values or NaN is NOT fitted (out_k[side] = 0): np.argsort's tie order
 * decides its weights, so the caller fits it with tpe_host_fit_parzen and
 * numpy's permutation.  out: 6 rows of n + 1 doubles — below w, mu, sigma,
 * above w, mu, sigma; out_k[0] / out_k[1] = below / above component counts. */
int tpe_host_fit_split(const double* x, const int64_t* tids, const int64_t* order, int64_t n,
                       const int64_t* below_tids, int64_t n_bt, double prior_weight, double prior_mu,
                       double prior_sigma, int32_t lf, double* out, int64_t* out_k);

/* categorical posterior (tpe.py:573-607): p_prior NULL = randint pseudo-counts,
 * else pchoice's counts + upper * prior_weight * p_prior */
int tpe_host_cat_probs(const int64_t* obs, int64_t n, int32_t upper, const double* p_prior, double prior_weight,
                       int32_t lf, double* out);

/* ap_filter_trials + the categorical posteriors of both sides of one label
 * (tpe.py:613-641, 573-607): obs/tids in strictly ascending tid order,
 * below_tids ascending; out_below / out_above: `upper` probabilities each */
int tpe_host_cat_split(const int64_t* obs, const int64_t* tids, int64_t n, const int64_t* below_tids, int64_t n_bt,
                       int32_t upper, const double* p_prior, double prior_weight, int32_t lf, double* out_below,
                       double* out_above);

/* ------------------------------------------------------------------------
 * Exact-replay candidate draws (host): numpy's legacy RandomState stream —
 * MT19937 (the 624-word key and position of RandomState.get_state()),
 * random_sample's 53-bit double, the polar-method gauss with its cached
 * second value, and multinomial(n=1, p) as numpy computes it (a binomial by
 * inversion per category, p_j over the remaining mass, until the draw is
 * placed).  The state is read and written in place, so draws interleave with
 * the caller's own use of the same RandomState.  Reference call sites:
 * tpe.py:73-74 / :224-231 (unbounded: n multinomials, then n normals),
 * tpe.py:82-87 / :240-244 (bounded: multinomial + normal per draw, rejected
 * outside [low, high)), pyll/stochastic.py:126-131 (categorical).
 * ---------------------------------------------------------------------- */
typedef struct tpe_mt_state {
  uint32_t key[624];
  int32_t pos;           /* next key word (624: regenerate first)        */
  int32_t has_gauss;     /* a cached second polar-method value is pending */
  double gauss;
} tpe_mt_state;

/* n draws from the mixture (w, mu, sigma)[k]: the normal deviate d of each
 * accepted draw (bounded: low <= d < high, in the mixture's own coordinate —
 * the caller applies exp / rounding, vectorised, as the reference does);
 * TPE_E_ARG on bad weights (numpy raises ValueError) */
int tpe_replay_mixture(tpe_mt_state* st, const double* w, const double* mu, const double* sigma, int64_t k,
                       int32_t bounded, double low, double high, int64_t n, double* out);

/* n categorical draws (one multinomial(1, p) row each): the chosen index */
int tpe_replay_categorical(tpe_mt_state* st, const double* p, int64_t k, int64_t n, int64_t* out);

/* pack one tree level into `blob` (all tables, 256-B aligned, ready for one
 * host->device copy); TPE_E_SPACE (info->blob_bytes = size needed) if too small */
int tpe_host_pack_level(const tpe_label_in* labels, int32_t n_labels, int32_t n_cand, uint64_t seed,
                        int64_t cand_base, int64_t n_cand_global, int32_t precision, void* blob, int64_t blob_cap,
                        tpe_pack_info* info);

/* ------------------------------------------------------------------------
 * One-call level runner: pack (host) -> H2D -> fit/sample/sort/score/select ->
 * D2H of the per-problem results -> stream synchronise.  This is the whole
 * per-tree-level device round trip of tpe.suggest (tpe.py:663-701 for every
 * active hyperparameter of the level) behind one C call, so the host language
 * pays one foreign call per level.  All memory is caller-owned; the runner
 * never allocates.
 * ---------------------------------------------------------------------- */
typedef struct tpe_level_ws {
  void* pinned; int64_t pinned_bytes;          /* page-locked host staging (tables + result readback) */
  void* pinned_dev;                            /* its device address (tpe_pinned_device_address), or NULL:
                                                  looked up by the call                                 */
  void* blob; int64_t blob_bytes;              /* device copy of the packed tables                      */
  double* cand; float* coord;                  /* device candidate pools, cand_cap elements each        */
  uint32_t* keys; uint64_t* vals; uint32_t* keys_sorted; uint64_t* vals_sorted; int64_t cand_cap;
  void* sort_tmp; int64_t sort_tmp_bytes;
  double* part; int64_t part_cap;              /* elements                                              */
  tpe_best* tile_best; int64_t best_cap;       /* elements                                              */
  tpe_result* result; int64_t result_cap;      /* elements (device)                                     */
  double* fit_keys; double* fit_keys_sorted;
  uint32_t* fit_vals; uint32_t* fit_vals_sorted; int64_t fit_cap;   /* elements                    */
  double* draw_pref; int64_t draw_pref_cap;    /* elements                                              */
  unsigned long long* pool_best; int64_t pool_best_cap;   /* elements                                   */
  void* tab; int64_t tab_cap;                  /* score tables, 16-B units                              */
} tpe_level_ws;

/* what a level needs (written on success and on TPE_E_SPACE) */
typedef struct tpe_level_need {
  int64_t pinned_bytes, blob_bytes, cand, sort_tmp_bytes, part, best, result, fit, draw_pref, pool_best, tab;
} tpe_level_need;

/* Run one tree level: `labels` as for tpe_host_pack_level; `out` receives one
 * tpe_result per (label, id) in order.  TPE_E_SPACE: a workspace is too small —
 * `need` holds every size; grow and call again (nothing was launched). */
int tpe_level_run(const tpe_label_in* labels, int32_t n_labels, int32_t n_cand, uint64_t seed, int64_t cand_base,
                  int64_t n_cand_global, int32_t precision, int32_t flags, const tpe_level_ws* ws,
                  tpe_level_need* need, void* stream, tpe_result* out);

/* ------------------------------------------------------------------------
 * One native call per tpe.suggest of a conditional (hp.choice) tree space:
 * the below/above split and Parzen fit of every label it needs
 * (ap_filter_trials + adaptive_parzen_normal / the categorical posteriors,
 * tpe.py:613-641, 398-607), the speculative fusion of the tree levels (gate
 * winners predicted from the fitted categorical posteriors, every level in one
 * device batch, predictions verified on the results; level by level on a
 * misprediction — the activity rule of vectorize.py:19-37 /
 * pyll/base.py:762-781), and the level runs (tpe_level_run).  The host keeps
 * only the history view and the trial documents.
 *
 * Covered: continuous (GAUSS / LOGGAUSS) and categorical labels fitted on the
 * host at TPE_PREC_F32, categorical gates, and any label whose fit the caller
 * supplies (host_w/mu/sigma/k).  A label the tree needs that it cannot fit —
 * quantized labels and sides with repeated values (numpy's argsort tie order
 * decides their weights), missing value orders (NaN) — is flagged in need_fit
 * and TPE_E_FALLBACK returned: the caller fits those labels (exactly as the
 * reference) and calls again with their fits.  Continuous labels large enough
 * for the device Parzen fit run it (tpe_fit_above) when their record carries
 * the device column; without it, and with non-categorical gates, the call
 * returns TPE_E_FALLBACK with no flag before any fit or run: the caller takes
 * its general path.  (On TPE_E_FALLBACK nothing is written; a device batch may
 * have run when a deeper level flagged a label.)
 * ---------------------------------------------------------------------- */
#define TPE_TREE_MAX_PARENTS 4
enum { TPE_E_FALLBACK = -5 };

/* one hyperparameter of the tree, in label order (label_ix = its position).
 * Quantized labels and continuous sides with repeated values are fitted with
 * numpy's argsort permutation of each side (its tie order decides the linear-
 * forgetting weights of tied observations, tpe.py:427-428): the caller passes
 * those permutations (side_order) with the fit coordinate, or gets need_fit. */
typedef struct tpe_tree_label {
  int32_t family, flags, upper, label_ix;   /* family: TPE_FAM_*; flags: TPE_F_HAS_LOW / TPE_F_HAS_HIGH */
  double low, high;                         /* sampling-space bounds (log space for LOGGAUSS)           */
  double prior_mu, prior_sigma;             /* adaptive_parzen_normal prior (continuous)                */
  const double* p_prior;                    /* categorical: pchoice probabilities (NULL: randint)       */
  const int64_t* tids;                      /* observation tids, strictly ascending                     */
  const void* values;                       /* continuous: f64 kernel coordinate (x, or ln x for
                                               LOGGAUSS); categorical: int64 categories                 */
  const int64_t* order;                     /* continuous: permutation sorting `values` ascending        */
  int64_t n_obs;
  int32_t depth, n_parents;                 /* tree level (roots 0); 0 parents = unconditional           */
  int32_t parent[TPE_TREE_MAX_PARENTS];     /* active iff some parent[j] (a label index) chose          */
  int32_t parent_cat[TPE_TREE_MAX_PARENTS]; /* category parent_cat[j]                                   */
  double q;                                 /* quantum of the quantized families (else 0)                */
  const double* host_w[2];                  /* a caller-made fit, [0] below / [1] above (host_k[0] > 0):  */
  const double* host_mu[2];                 /* used as is (categorical: host_w = the probabilities)     */
  const double* host_sigma[2];
  int64_t host_k[2];
  /* device Parzen fit of the above side (continuous labels with n_obs >= device_fit_min): the
   * label's device column (n_obs kernel coordinates in tid order) and its resident value order
   * (tpe_label_in); NULL dev_obs: such a label sends the space to the caller's general path */
  const double* dev_obs;
  const double* ord_key_in; const uint32_t* ord_idx_in; int64_t n_ord_in;
  double* ord_key_out; uint32_t* ord_idx_out;
  /* the caller's sort of each side (continuous and quantized families): side_order[s] = numpy's
   * np.argsort of side s's coordinates in tid order (s = 0 below, 1 above; `values` = the
   * fit coordinate, e.g. log(max(x, max(EPS, e^low))) for qloguniform, tpe.py:517-568), side_n[s]
   * its length (checked against the split made here).  Both set: the label is fitted here with
   * those permutations — the reference's tie order — instead of being sent to the caller
   * (need_fit).  NULL: the label's own rules above. */
  const int64_t* side_order[2];
  int64_t side_n[2];
} tpe_tree_label;

/* tpe_suggest_tree flags: the tpe_level_run flags, plus */
enum { TPE_TREE_NO_SPECULATE = 1 << 8 };    /* level by level only (no fused batch)                    */

/* ------------------------------------------------------------------------
 * Candidate-shard exchange (multi-GPU, one process per GPU).  A sharded
 * suggest gives every rank the contiguous global candidate range
 * [cand_base, cand_base + n_cand) of each problem (Philox counters are global
 * indices, so the candidates are the ones a single GPU draws there).  After
 * each level run, the ranks all-gather their per-problem results — a header
 * with the rank's status, then P tpe_result records — and every rank reduces
 * them to the global winners with np.argmax semantics (NaN first, then the
 * largest score, then the lowest global index; the reference's per-parameter
 * argmax, tpe.py:749-759), so every rank takes the same tree decisions.  A
 * rank whose level run needs a larger workspace still takes part (status
 * TPE_E_SPACE, empty results) and then every rank returns TPE_E_SPACE: the
 * callers grow and call again in lock-step.
 * The all-gather is an RCCL all-gather over xGMI on the device scratch `dev`
 * when `comm` is set (tpe_comm_init), else the caller's host all-gather.
 * ---------------------------------------------------------------------- */
#define TPE_COMM_ID_BYTES 128
#define TPE_EXCHANGE_HEADER 64   /* bytes before a rank's result records in the exchange */
typedef int (*tpe_gather_fn)(void* ctx, const void* mine, int64_t bytes, void* all);
typedef struct tpe_exchange {
  int32_t rank, world;
  void* comm;             /* RCCL communicator (tpe_comm_init), or NULL                          */
  tpe_gather_fn gather;   /* host all-gather: `bytes` from every rank into all[world * bytes], in
                             rank order; returns 0 on success (used when comm is NULL)          */
  void* ctx;
  void* dev; int64_t dev_bytes;   /* RCCL path: device scratch of world * (TPE_EXCHANGE_HEADER +
                                     P * sizeof(tpe_result)) bytes for the largest level          */
  int32_t always;         /* exchange even when world == 1 (tests of the exchange itself)       */
  int32_t reserved;
} tpe_exchange;

/* RCCL communicator of one process per GPU: rank 0 makes the id, the caller
 * broadcasts its TPE_COMM_ID_BYTES bytes, every rank calls tpe_comm_init on
 * its device.  librccl is loaded on first use (no link-time dependency). */
int tpe_comm_unique_id(void* id);
int tpe_comm_init(int32_t rank, int32_t world, const void* id, int32_t device, void** comm);
int tpe_comm_destroy(void* comm);

/* ------------------------------------------------------------------------
 * Device column store (hyperopt_amd/devhist.py; ABI 22).  The observation
 * columns of device-fitted labels are segments of one flat float64 store.
 * tpe_scatter_f64: dst[pos[i]] = val[i] for the k appended observations of a
 * suggest; `src` is the DEVICE address (tpe_pinned_device_address) of pinned
 * host memory holding k doubles then k int64 positions, read by the kernel
 * itself (no copy): the caller keeps it unchanged until the stream has passed
 * the launch.  tpe_move_ranges: a re-layout of a store (or of the value
 * orders' key / position buffers, elem_bytes 8 / 4): for each of n_ranges
 * {src_off, dst_off, n} int64 triples (pinned, device-addressable, as above)
 * dst[dst_off + i] = src[src_off + i], i < n; src and dst distinct buffers.
 * ---------------------------------------------------------------------- */
int tpe_scatter_f64(const void* src, int64_t k, double* dst, void* stream);
int tpe_move_ranges(const void* ranges, int32_t n_ranges, int32_t elem_bytes, const void* src, void* dst,
                    void* stream);

/* collectives (ncclAllGather calls) this library has issued in this process,
 * in *n: the device combine of candidate-sharded levels and
 * tpe_exchange_allgather over RCCL.  A one-rank exchange (world 1, `always`)
 * issues its in-place all-gather only under TPE_FORCE_COMBINE=1 (the N-rank
 * combine run on one GPU: tests), else the gather is the identity and is
 * skipped.  (ABI 22) */
int tpe_collectives_issued(int64_t* n);

/* the exchange's reduction on the host: all[world][P] -> out[P], np.argmax
 * order over (score, global_idx), empty records (idx < 0) skipped */
int tpe_combine_results(const tpe_result* all, int32_t world, int64_t P, tpe_result* out);

/* ------------------------------------------------------------------------
 * Shard axes.  Besides the candidate axis above, a batched suggest shards
 * with no exchange inside the suggest:
 *   new-id axis          every new id is an independent suggest on the same
 *                        history (the reference's one-id call, tpe.py:812,
 *                        repeated): rank r takes a contiguous block of the ids;
 *   hyperparameter axis  broadcast_best is per hyperparameter
 *                        (tpe.py:749-759): rank r evaluates the non-gate labels
 *                        it owns, every rank evaluates the gates (so every rank
 *                        knows which labels are active), the others are
 *                        TPE_F_REMOTE.
 * Candidates are keyed on (seed, label, new id, global index), so each rank
 * computes exactly what one device computes for its part.  The chosen values
 * are then all-gathered once (tpe_exchange_allgather) and every rank holds
 * the whole result.
 * ---------------------------------------------------------------------- */

/* all-gather of `bytes` host bytes per rank through the exchange: all[world *
 * bytes] in rank order.  RCCL (ex->comm): the bytes go through ex->dev (at
 * least world * bytes) on `stream` — one copy in, an in-place ncclAllGather, one
 * copy out, a stream synchronise; else ex->gather.  Rank-collective. */
int tpe_exchange_allgather(const tpe_exchange* ex, const void* mine, int64_t bytes, void* all, void* stream);

/* below_tids ascending (the n_below best trials, tpe.py:625-629); ids: the
 * n_ids new trial ids; n_cand candidates per problem on this rank, global
 * indices [cand_base, cand_base + n_cand) of n_cand_global (unsharded: 0, 0);
 * ex: the shard exchange (NULL unsharded); speculate_min_draws: a gate is
 * predicted when its predicted category is expected among >= this many of the
 * n_cand_global draws;
 * device_fit_min > 0: continuous labels with that many observations get the
 * device Parzen fit of their above side (their below side, <= 25 observations
 * with equal weights, is fitted here) when the record carries dev_obs, else the
 * space is left to the caller's general path.  values / active: [n_ids x n_labels] — the chosen
 * value (categories as doubles) and whether the label is active; path[0] = 1
 * when the fused batch was used, path[1] = level runs issued; need_fit
 * [n_labels]: set to 1 for the labels the caller must fit (TPE_E_FALLBACK).
 * TPE_E_SPACE: grow the workspace to `need` and call again. */
int tpe_suggest_tree(const tpe_tree_label* labels, int32_t n_labels, const int64_t* below_tids, int64_t n_below,
                     double prior_weight, int32_t lf, const int64_t* ids, int32_t n_ids, int32_t n_cand,
                     int64_t cand_base, int64_t n_cand_global, const tpe_exchange* ex,
                     uint64_t seed, double speculate_min_draws, int64_t device_fit_min, int32_t flags,
                     const tpe_level_ws* ws, tpe_level_need* need, void* stream, double* values, int8_t* active,
                     int32_t* path, int8_t* need_fit);

/* Host worker threads of the native runtime, the calling thread included
 * (default: TPE_HOST_THREADS, else 16 — at most the host's CPUs; at most 16).  tpe_suggest_tree fits the
 * labels of a suggest on them in parallel (each label's fit is the same
 * single-threaded computation wherever it runs, so results do not depend on
 * the count).  n <= 1: everything on the calling thread; n < 0: query only.
 * *previous (if not NULL) gets the count before the call.  Not to be called
 * while another thread is inside tpe_suggest_tree. */
int tpe_host_threads(int32_t n, int32_t* previous);

/* ------------------------------------------------------------------------
 * Stage profiler of tpe_level_run (bench.py's live roofline).  While enabled,
 * the runner brackets each stage it calls with HIP events on its own stream and,
 * after its stream synchronise, keeps the per-stage device times of that run.
 * The stages are timed exactly as the production flow issues them: a stage
 * that launches nothing (no fits, no sort, early selection leaving no late
 * problems for the select stage) reports launches = 0 and ms = 0.
 * Process-wide setting; not meant for concurrent runners.
 * ---------------------------------------------------------------------- */
#define TPE_STAGE_FIT      0
#define TPE_STAGE_TABLES   1
#define TPE_STAGE_SAMPLE   2
#define TPE_STAGE_SORT     3
#define TPE_STAGE_ABOVE    4
#define TPE_STAGE_FINALIZE 5
#define TPE_STAGE_SELECT   6
#define TPE_N_STAGES       7

typedef struct tpe_stage_prof {
  double ms;         /* device time between the stage's bracketing events         */
  double units;      /* stage work: fit scratch slots | table units (16 B) |
                        candidates drawn by the sample kernels (lazy categoricals,
                        scanned by the table stage, excluded) | sort bytes (8-bit
                        LSD passes x 2 x 12 B x keys) | above CE | candidates |
                        problems                                                    */
  double ce;         /* algorithmic component evaluations the stage stands in for:
                        sample = tabulated problems' (K_below + K_above) x C,
                        above = scored problems' K_above x C; else 0                */
  int32_t launches;  /* kernels (and library sorts) the stage launched             */
  int32_t kernel_ns; /* sample stage: its tabulated pass's kernel alone, timed by the
                        start / stop events of its own launch (hipExtLaunchKernel) on
                        the stage's stream, in ns; 0 where not timed               */
} tpe_stage_prof;

/* enable (1) / disable (0) the profiler; creates its events on first use */
int tpe_level_profile(int32_t enable);

/* Debug (tests): while `dev` is set, the sample stage's k_sample_fast pass also
 * writes every candidate's {value, l, g, label index} as four doubles at
 * dev[4 * (cand_off + i)] (device memory, n_records >= the level's candidates;
 * the run records are unchanged).  NULL: the production kernel.  Process-wide. */
int tpe_debug_fast_lg(void* dev, int64_t n_records);

/* the last profiled tpe_level_run: min(n, TPE_N_STAGES) records in stage
 * order; TPE_E_ARG if no run completed since the profiler was enabled */
int tpe_level_profile_read(tpe_stage_prof* out, int32_t n);

/* ------------------------------------------------------------------------
 * Candidate report (tpe_report.hip; ABI 23): the k best DISTINCT candidate
 * values of every problem of a batch and statistics of its scores, computed
 * from the per-candidate buffers a tpe_run_batch with TPE_BATCH_WRITE_CAND,
 * l_out and g_out leaves on the device (cand, l_out, g_out: all indexed
 * cand_off + i by original candidate index).  Of a problem the stage reads
 * n_cand, cand_off and cand_base only.
 *
 * Score s = l - g (float64).  Ranked order = np.argmax order (tpe_select): NaN
 * scores first (equal to each other), then descending (+-inf ordinary values),
 * ties to the lower candidate index.  Walking that order, a candidate is kept
 * when no kept candidate has an equal (float64 ==) value; the first k kept are
 * the problem's entries top[p * k ..], n_top[p] = min(k, distinct values) their
 * count; the entries after them are {0, 0, 0, -1}.
 * Statistics: the counts of finite, NaN, +inf and -inf scores; mean, m2 =
 * sum (s - mean)^2, min and max over the finite ones (none: mean, min, max =
 * NaN, m2 = 0).  mean is the Monte-Carlo estimate of E_l[log l - log g] over
 * the candidate pool (the candidates are draws from l).
 *
 * Two passes.  A problem's candidates are cut into chunks of TPE_REPORT_CHUNK
 * consecutive indices; pass 1 (one workgroup per problem and chunk) writes the
 * chunk's distinct top-k and its (n, mean, m2, min, max) record to `scratch`,
 * pass 2 (one workgroup per problem) merges the lists by the same rule — a
 * chunk's distinct top-k holds every entry of the problem's that lies in the
 * chunk — and the records by Chan's update in a fixed order.  No float atomics:
 * two calls on the same buffers give the same bytes.
 *
 * Chunk slots: every problem gets S = ceil(ceil(total_cand / n_problems) /
 * TPE_REPORT_CHUNK) of them — a packed level gives every problem the same
 * n_cand and total_cand = n_problems * n_cand — so n_chunks_total =
 * n_problems * S, and tpe_report_scratch_bytes(n_chunks_total, k) =
 * n_chunks_total * (80 + 32 k).  A problem that does not fit (n_cand > S *
 * TPE_REPORT_CHUNK, or [cand_off, cand_off + n_cand) outside [0, total_cand))
 * is not read: n_top[p] = -1, empty statistics.
 *
 * tpe_report returns TPE_E_ARG before any launch (no device needed) for a null
 * batch, k outside [1, TPE_REPORT_MAX_K], null cand / l_out / g_out,
 * TPE_BATCH_WRITE_CAND not set, null outputs, or scratch smaller than
 * tpe_report_scratch_bytes.  Pooled problems (TPE_F_POOLED) are not supported;
 * the problem flags live in device memory, so the CALLER checks its host copy
 * of them before the call (hyperopt_amd.engine.Engine.run does, and raises).
 * ---------------------------------------------------------------------- */
#define TPE_REPORT_CHUNK 4096
#define TPE_REPORT_MAX_K 64
typedef struct tpe_top_entry {
  double value, l, g;
  int64_t global_idx;    /* cand_base + candidate index */
} tpe_top_entry;
typedef struct tpe_score_stats {
  int64_t n_finite, n_nan, n_posinf, n_neginf;
  double mean, m2, min, max;
} tpe_score_stats;

int tpe_report_scratch_bytes(int64_t n_chunks_total, int32_t k, uint64_t* bytes);

/* top: device [n_problems * k]; n_top: device [n_problems]; stats: device
 * [n_problems]; enqueued on `stream` after the batch's stages */
int tpe_report(const tpe_batch* batch, int32_t k, tpe_top_entry* top, int32_t* n_top, tpe_score_stats* stats,
               void* scratch, uint64_t scratch_bytes, void* stream);

/* Profiling only (tools/report_time.py).  While enabled, tpe_report launches its
 * two kernels with start / stop events of their own; last_ms (if not NULL)
 * first gets the device times {pass 1, pass 2} in ms of the last such call —
 * it WAITS for that call's kernels — then the setting changes.  Process-wide. */
int tpe_report_profile(int32_t enable, double* last_ms);

/* ------------------------------------------------------------------------
 * Joint candidate report (tpe_report.hip; ABI 24, symbols added): the k best
 * DISTINCT candidate ROWS of every problem of a joint stage and the statistics
 * of its scores, from the buffers tpe_joint_run, tpe_joint_mixed_run,
 * tpe_joint_quant_run, tpe_joint_wide_run or tpe_joint_seg_run leave on the
 * device: cand (f32, problem p's n_cand rows of width_p floats, row-major, from
 * element cand_off[p] on; cand_off == NULL: p * n_cand * width), l_out and
 * g_out (f64 [n_probs * n_cand]).  The stage takes arbitrary l and g: it never
 * assumes that equal rows have equal scores.
 *
 * Score s = l - g (float64).  Ranked order = np.argmax order, as "Candidate
 * report": NaN scores first (equal to each other), then descending (+-inf
 * ordinary values), ties to the lower candidate index.  Walking that order, a
 * candidate is kept when no kept candidate has an equal row.  Two rows are
 * equal iff all width_p f32 coordinates compare ==: -0 equals +0, a row with a
 * NaN coordinate equals nothing (not even itself: every such candidate is
 * kept).  The first k kept are the problem's entries top[p * k ..] = {candidate
 * index, l, g, 0}, n_top[p] = min(k, distinct rows) their count; entry r's row
 * is copied (bit for bit) to top_z[(p * k + r) * z_stride ..], the floats from
 * width_p to z_stride are 0.  The entries after n_top[p] are {-1, 0, 0, 0} with
 * zero rows.  Statistics: tpe_score_stats, exactly as "Candidate report".
 *
 * Two passes, as tpe_report.  Pass 1: one 256-thread workgroup per (problem,
 * chunk of TPE_JOINT_REPORT_CHUNK consecutive candidates); a lane keeps the
 * score keys and a 32-bit row hash of its 16 candidates in registers.  Equal
 * rows have equal hashes (-0 hashed as +0), so the hash only filters which
 * rows are re-read from `cand` and compared, coordinate by coordinate, with
 * the round winner's row in LDS: the hash never decides equality.  The chunk
 * statistics: per-lane two-pass, a butterfly with the lower lane first, the
 * waves in order.  Pass 2: one workgroup per problem merges the chunk lists
 * (ranked and distinct, so only list heads compete; a chunk's list holds every
 * entry of the problem's that lies in the chunk) against the chosen rows held
 * in LDS (k * width floats, at most 16 KB), and the chunk statistics by Chan's
 * update in chunk order.  No float atomics, every reduction has a fixed shape:
 * two calls on the same buffers give the same bytes.
 *
 * tpe_joint_report_scratch_bytes(n_probs, n_cand, k) = n_probs * S * (80 +
 * 32 k), S = ceil(n_cand / TPE_JOINT_REPORT_CHUNK).
 *
 * tpe_joint_report returns TPE_E_ARG before any launch (no device needed) for
 * null args, buffers or outputs, k outside [1, TPE_REPORT_MAX_K], n_probs < 1,
 * n_cand < 1, a width outside [1, TPE_JOINT_WIDE_MAX_DIMS], z_stride below the
 * largest width, `widths` without `host_widths`, n_probs * S beyond int32, or
 * scratch smaller than tpe_joint_report_scratch_bytes.
 * ---------------------------------------------------------------------- */
#define TPE_JOINT_REPORT_CHUNK 4096
typedef struct tpe_joint_top_entry {
  int64_t idx;           /* candidate index in the problem's pool; -1: unused entry */
  double l, g;
  int64_t reserved;      /* 0 */
} tpe_joint_top_entry;
typedef struct tpe_joint_report_args {
  int32_t n_probs, n_cand, width, z_stride;   /* width: every problem's row width when widths == NULL */
  const float* cand;           /* device */
  const double *l_out, *g_out; /* device [n_probs * n_cand] */
  const int64_t* cand_off;     /* device [n_probs] element offsets into cand; NULL: p * n_cand * width */
  const int32_t* widths;       /* device [n_probs], each in [1, 64]; NULL: `width` */
  const int32_t* host_widths;  /* host copy of widths for the argument check (NULL with widths == NULL) */
} tpe_joint_report_args;

int tpe_joint_report_scratch_bytes(int32_t n_probs, int32_t n_cand, int32_t k, uint64_t* bytes);

/* top: device [n_probs * k]; top_z: device f32 [n_probs * k * z_stride]; n_top:
 * device [n_probs]; stats: device [n_probs]; enqueued on `stream` (after the
 * joint stage that wrote the buffers) */
int tpe_joint_report(const tpe_joint_report_args* args, int32_t k, tpe_joint_top_entry* top, float* top_z,
                     int32_t* n_top, tpe_score_stats* stats, void* scratch, uint64_t scratch_bytes, void* stream);

/* tpe_report_profile for tpe_joint_report (tools/joint_report_time.py) */
int tpe_joint_report_profile(int32_t enable, double* last_ms);

/* ------------------------------------------------------------------------
 * Joint (multivariate) TPE stage (tpe_joint.hip; ABI 24): candidates are whole
 * vectors z[D] (D <= TPE_JOINT_MAX_DIMS kernel coordinates: the value, or its
 * log for the log families), a mixture component is a product of D normals
 * truncated to the labels' bounds, one argmax per new id picks the vector.
 * Nothing on the univariate suggest path runs through this stage.
 *
 * Density rows of a side (below: l, above: g), K components, all f32, device:
 *   mu[K * D]   component k, dimension d at [k * D + d]
 *   a [K * D]   sqrt(log2(e) / 2) / sigma_kd
 *   c [K]       log2 of  w_k / prod_d (sigma_kd sqrt(2 pi) mass_kd),
 *               mass_kd = Phi((high_d - mu_kd) / sigma_kd) - Phi((low_d - mu_kd) / sigma_kd)
 *               (1 where unbounded), shifted so that max_k c_k = 0
 *   base        (double) the shift in natural-log units (parzen.gauss_table's scheme)
 *   log p(z) = ln2 * log2( sum_k 2^(c_k - sum_d (a_kd (z_d - mu_kd))^2) ) + base
 * The sum over d is accumulated in this subtract-then-scale form in f32; the
 * sum over k carries a running maximum per candidate, so a candidate more than
 * 126 binades below max c still gets a finite density.  score = l - g in f64.
 *
 * Sampler rows of the below side, device:
 *   samp_cum[K_below]           (double) cumsum of the normalised weights, last = 1
 *   samp[(k * D + d) * 5 + ..]  (float) {mu, sigma, fa, fb, flip}: fa, fb = Phi of
 *                               the standardised bounds, mirrored (flip != 0) when
 *                               the interval lies right of 0 (parzen.sampler_table)
 * Candidate i of new id j (i < n_cand < 2^31): Philox-4x32-10 with key =
 * (seed lo, seed hi) and counter = (i, b, stream_word, id_j lo), b = 0, 1, ...
 * the block number.  The candidate's words in block order: word 0 -> u01w -> the
 * component k (first k with u < samp_cum[k]); word 1 + d -> the 23-bit uniform
 * u of dimension d, z_d = mu_kd + sigma_kd * ndtri_f32(fa + u (fb - fa)) (negated
 * under flip), clipped to [smallest float >= low_d, largest float < high_d].
 * stream_word must differ from every univariate label index (tpe_problem.ctr2):
 * TPE_JOINT_STREAM.
 *
 * One 256-thread workgroup per (id, chunk of TPE_JOINT_CHUNK consecutive
 * candidates) samples (or loads, TPE_JOINT_INJECT) its candidates into
 * registers, streams both sides' rows through LDS, and writes its chunk winner
 * to `scratch`; a second launch merges an id's chunks in index order.  Winner =
 * np.argmax order of score (NaN first, ties to the lower index).  No atomics:
 * the same call twice gives the same bytes.
 *
 * tpe_joint_run returns TPE_E_ARG before any launch (no device needed) for null
 * args / rows / ids / records, n_dims outside [1, TPE_JOINT_MAX_DIMS],
 * n_cand < 1, n_ids < 1, k_below < 1, k_above < 1, TPE_JOINT_INJECT without
 * `inject`, or scratch smaller than tpe_joint_scratch_bytes(n_ids, n_cand).
 * ---------------------------------------------------------------------- */
#define TPE_JOINT_MAX_DIMS 16
#define TPE_JOINT_CHUNK 1024
#define TPE_JOINT_STREAM 0xFFFFFFFFu
#define TPE_JOINT_INJECT 1     /* tpe_joint_args.flags: score `inject` instead of sampling */
typedef struct tpe_joint_record {
  int64_t global_idx;          /* the winner's candidate index */
  double l, g;
  double z[TPE_JOINT_MAX_DIMS];   /* its coordinates (entries from n_dims on: 0) */
} tpe_joint_record;
typedef struct tpe_joint_args {
  int32_t n_dims, n_cand, n_ids, flags;
  int32_t k_below, k_above;
  uint32_t stream_word;
  int32_t reserved;
  uint64_t seed;
  const float *below_mu, *below_a, *below_c;
  const float *above_mu, *above_a, *above_c;
  double below_base, above_base;
  const double* samp_cum;
  const float* samp;
  const int64_t* ids;          /* device [n_ids] */
  const float* inject;         /* device [n_cand * n_dims], every id scores it */
  double low[TPE_JOINT_MAX_DIMS], high[TPE_JOINT_MAX_DIMS];   /* -inf / +inf: unbounded */
} tpe_joint_args;

int tpe_joint_scratch_bytes(int32_t n_ids, int32_t n_cand, uint64_t* bytes);

/* records: device [n_ids]; optional (NULL: not written) cand: device f32
 * [n_ids * n_cand * n_dims], l_out / g_out: device f64 [n_ids * n_cand];
 * enqueued on `stream` */
int tpe_joint_run(const tpe_joint_args* args, tpe_joint_record* records, float* cand, double* l_out, double* g_out,
                  void* scratch, uint64_t scratch_bytes, void* stream);

/* Profiling only (tools/joint_time.py), as tpe_report_profile: last_ms gets the
 * device times {chunk kernel, merge kernel} of the last profiled tpe_joint_run,
 * tpe_joint_mixed_run, tpe_joint_quant_run, tpe_joint_wide_run,
 * tpe_joint_seg_run or tpe_joint_wide_seg_run (a segmented run's first entry
 * sums its launches before the merge; the wide one's without its sampler). */
int tpe_joint_profile(int32_t enable, double* last_ms);

/* ------------------------------------------------------------------------
 * Wide joint stage (tpe_joint.hip; additive to ABI 24): the stage above for a
 * group of up to TPE_JOINT_WIDE_MAX_DIMS continuous labels.  The model, the
 * density and sampler rows, the score and the winner's order are those of
 * tpe_joint_run; only where the data lives differs, and the record and the
 * bounds are 64 wide.  64 bounds the set of kernel instantiations (padded
 * widths 20, 24, 32, 48, 64); it is a condition, not a measurement.
 *
 * The Philox streams are tpe_joint_run's, continued: word 1 + d of candidate i
 * serves dimension d, that is word (1 + d) & 3 of block (1 + d) >> 2 (D = 64:
 * blocks 0 to 16).  A wide run and a tpe_joint_run over the same model cut to
 * its first D' <= TPE_JOINT_MAX_DIMS dimensions (same seed, stream_word and
 * ids) draw the same f32 coordinates in those dimensions, bit for bit.
 *
 * Three launches: k_joint_wide_sample (skipped under TPE_JOINT_INJECT) draws
 * one candidate a thread in a loop over d and writes it to `scratch`, laid out
 * [256-candidate block][d][256] so that its stores and the scoring kernel's
 * loads are coalesced; k_joint_wide_chunk<DP, R> (one workgroup per id and
 * chunk of 256 R candidates, R = 2 for DP <= 32 and 1 above) loads them into
 * registers and scores them as k_joint_chunk does, both sides' rows streaming
 * through LDS in tiles of at most 32 KiB; k_joint_wide_merge picks an id's
 * winner from its chunks in index order.  No atomics: the same call twice
 * gives the same bytes.
 *
 * tpe_joint_wide_run accepts n_dims in [1, TPE_JOINT_WIDE_MAX_DIMS] (so it can
 * be compared with tpe_joint_run at n_dims <= TPE_JOINT_MAX_DIMS) and returns
 * TPE_E_ARG before any launch (no device needed) for everything tpe_joint_run
 * rejects, n_dims outside that range, or scratch smaller than
 * tpe_joint_wide_scratch_bytes(n_ids, n_cand, n_dims).
 * ---------------------------------------------------------------------- */
#define TPE_JOINT_WIDE_MAX_DIMS 64
typedef struct tpe_joint_wide_record {
  int64_t global_idx;          /* the winner's candidate index */
  double l, g;
  double z[TPE_JOINT_WIDE_MAX_DIMS];   /* its coordinates (entries from n_dims on: 0) */
} tpe_joint_wide_record;
typedef struct tpe_joint_wide_args {
  int32_t n_dims, n_cand, n_ids, flags;   /* as tpe_joint_args ... */
  int32_t k_below, k_above;
  uint32_t stream_word;
  int32_t reserved;
  uint64_t seed;
  const float *below_mu, *below_a, *below_c;
  const float *above_mu, *above_a, *above_c;
  double below_base, above_base;
  const double* samp_cum;
  const float* samp;
  const int64_t* ids;
  const float* inject;
  double low[TPE_JOINT_WIDE_MAX_DIMS], high[TPE_JOINT_WIDE_MAX_DIMS];   /* ... with 64 bounds */
} tpe_joint_wide_args;

/* the chunk records and the candidate block of one tpe_joint_wide_run */
int tpe_joint_wide_scratch_bytes(int32_t n_ids, int32_t n_cand, int32_t n_dims, uint64_t* bytes);

/* as tpe_joint_run: records device [n_ids]; optional cand device f32
 * [n_ids * n_cand * n_dims], l_out / g_out device f64 [n_ids * n_cand] */
int tpe_joint_wide_run(const tpe_joint_wide_args* args, tpe_joint_wide_record* records, float* cand, double* l_out,
                       double* g_out, void* scratch, uint64_t scratch_bytes, void* stream);

/* Profiling only: while tpe_joint_profile is enabled a sampling
 * tpe_joint_wide_run (tpe_joint_wide_mixed_run) also times k_joint_wide_sample
 * (k_joint_wide_mixed_sample); this reads that time (ms) of the last such run
 * (it WAITS for it). */
int tpe_joint_wide_profile(double* sample_ms);

/* ------------------------------------------------------------------------
 * Mixed joint stage (tpe_joint.hip; additive to ABI 24): a group of n_dims
 * continuous labels (0 allowed) and n_cat discrete ones (randint /
 * categorical), 1 <= n_dims + n_cat <= TPE_JOINT_MAX_DIMS.  Kernel coordinate
 * order: the continuous labels, then the discrete ones; a category travels as
 * its index (f32 in `cand` / `inject` / the component rows, double in
 * tpe_joint_record.z).  Everything tpe_joint_args says holds for the fields of
 * the same name (the rows of the continuous part: [K * n_dims]).
 *
 * Discrete dimension d has U_d = cat_upper[d] categories with prior p_d; its
 * tables start at cat_off[d] in the flat [sum_d U_d] tables (packed in
 * dimension order).  On a side with smoothing mass s_d a component k whose
 * category is x_kd >= 0 has  P_kd(v) = (1[v = x_kd] + s_d p_d(v)) / (1 + s_d);
 * a component whose category is -1 (the prior row) has P_kd(v) = p_d(v).
 *   cat  [K * n_cat]  (f32) x_kd at [k * n_cat + d], -1: never matches
 *   miss [total]      (f32) log2(s_d p_d(v) / (1 + s_d))
 *   bonus[total]      (f32) log2(1 + 1 / (s_d p_d(v)))
 *   c[K]              as tpe_joint_args, plus sum_d log2((1 + s_d) / s_d) over the
 *                     dimensions where x_kd = -1, before the shift to max 0
 *   log2 of a component's term at (z, v) = c_k - sum_cont(..) + sum_d [v_d = x_kd]
 *   bonus_d(v_d); the candidate's sum_d miss_d(v_d) is added in f64 after the
 *   sum over k.  A candidate's bonus_d(v_d) is read once per side, so a discrete
 *   dimension costs one compare, one select and one add per (candidate, component).
 *
 * Sampling: word 0 picks the component k and word 1 + j serves kernel
 * coordinate j, as in tpe_joint_run (so the continuous coordinates are those
 * of a tpe_joint_run over the continuous part).  A discrete coordinate takes
 * u = u01w(word): with h = below_h[d] = 1 / (1 + s_d) (h = 0 where x_kd = -1),
 * u < h gives v = x_kd, else v = the first category with (u - h) / (1 - h) <
 * cat_cum[cat_off[d] + v] (cat_cum: the cumsum of p_d, its last entry 1).
 *
 * tpe_joint_mixed_run returns TPE_E_ARG before any launch for everything
 * tpe_joint_run checks (mu / a / samp rows may be NULL when n_dims = 0),
 * n_cat < 0, n_dims < 0, n_dims + n_cat outside [1, TPE_JOINT_MAX_DIMS], a null
 * table while n_cat > 0, a U_d outside [2, TPE_JOINT_MAX_CATS], a category
 * total above TPE_JOINT_MAX_CAT_TOTAL, or a cat_off that leaves [0, total - U_d].
 * n_cat = 0 is tpe_joint_run on the same fields.  With TPE_JOINT_INJECT a
 * non-integral or out-of-range category in `inject` is the caller's error: the
 * device does not check it and the scores of such a candidate are unspecified.
 * tpe_joint_record, tpe_joint_scratch_bytes and tpe_joint_profile serve both.
 * ---------------------------------------------------------------------- */
#define TPE_JOINT_MAX_CATS 256          /* categories per discrete label */
#define TPE_JOINT_MAX_CAT_TOTAL 1024    /* categories per group */
typedef struct tpe_joint_mixed_args {
  int32_t n_dims, n_cand, n_ids, flags;   /* n_dims: the continuous labels */
  int32_t k_below, k_above;
  uint32_t stream_word;
  int32_t n_cat;                          /* the discrete labels */
  uint64_t seed;
  const float *below_mu, *below_a, *below_c;
  const float *above_mu, *above_a, *above_c;
  double below_base, above_base;
  const double* samp_cum;
  const float* samp;
  const int64_t* ids;
  const float* inject;                    /* device [n_cand * (n_dims + n_cat)] */
  double low[TPE_JOINT_MAX_DIMS], high[TPE_JOINT_MAX_DIMS];
  int32_t cat_upper[TPE_JOINT_MAX_DIMS];  /* U_d */
  int32_t cat_off[TPE_JOINT_MAX_DIMS];    /* start of dimension d in the flat tables */
  const float *below_cat, *above_cat;     /* device [K * n_cat] */
  const float *below_miss, *below_bonus;  /* device [total] */
  const float *above_miss, *above_bonus;
  const double* below_h;                  /* device [n_cat] */
  const double* cat_cum;                  /* device [total] */
} tpe_joint_mixed_args;

/* as tpe_joint_run; cand: device f32 [n_ids * n_cand * (n_dims + n_cat)] */
int tpe_joint_mixed_run(const tpe_joint_mixed_args* args, tpe_joint_record* records, float* cand, double* l_out,
                        double* g_out, void* scratch, uint64_t scratch_bytes, void* stream);

/* ------------------------------------------------------------------------
 * Wide mixed joint stage (tpe_joint.hip; additive to ABI 24): a group of n_dims
 * >= 1 continuous labels and 1 <= n_cat <= TPE_JOINT_WIDE_MAX_CAT discrete ones,
 * n_dims + n_cat <= TPE_JOINT_WIDE_MAX_DIMS.  Nothing is defined anew:
 *   model        that of the mixed joint stage above at a larger width: the
 *                weights, mu, sigma and smoothing masses of a side, P_kd(v) with
 *                s_d = prior_weight * U_d / (n + 1), in the device form miss_d /
 *                bonus_d; the prior row carries category -1.  Every table and
 *                row of tpe_joint_mixed_args means the same here.
 *   coordinates  the n_dims continuous labels, then the n_cat discrete ones; a
 *                category travels as its index (f32 in `cand` / `inject` / the
 *                component rows, double in tpe_joint_wide_record.z).
 *   streams      word 0 of block 0 picks the component; word 1 + j serves kernel
 *                coordinate j, that is word (1 + j) & 3 of block (1 + j) >> 2
 *                (stream_word and the new id as in tpe_joint_run).  A continuous
 *                coordinate is drawn as tpe_joint_wide_run draws it, a discrete
 *                one as tpe_joint_mixed_run does: u = u01w(word) in f64, h =
 *                below_h[d] (0 for a component of category -1), u < h takes the
 *                component's category, else the first category with (u - h) /
 *                (1 - h) < cat_cum[cat_off[d] + v].
 * So the continuous coordinates of a run equal those of a tpe_joint_wide_run
 * over the continuous part alone (same seed, stream_word and ids), and a run at
 * n_dims + n_cat <= TPE_JOINT_MAX_DIMS draws the candidates of
 * tpe_joint_mixed_run, both bit for bit.
 *
 * Three launches: k_joint_wide_mixed_sample (skipped under TPE_JOINT_INJECT)
 * draws one candidate a thread into `scratch`, laid out [256-candidate block]
 * [j][256] over all n_dims + n_cat coordinates; k_joint_wide_mixed_chunk<DP, KP,
 * R> (DP the padded n_dims in {12, 16, 20, 24, 32, 48, 64}, KP the padded n_cat
 * in {1, 2, 4, 8}, R = 2 candidates a lane for DP <= 32 and 1 above) scores a
 * chunk of 256 R candidates, both sides streaming through LDS in component
 * tiles of mu[DP], a[DP], cat[KP] and c (under 37 KiB a workgroup); a
 * discrete slot costs one compare, one select and one add per (candidate,
 * component), and sum_d miss_d(v_d) is added in f64 after the sum over the
 * components.  k_joint_wide_merge picks the winner.  No atomics: the same call
 * twice gives the same bytes.  TPE_JOINT_WIDE_MAX_CAT bounds the set of kernel
 * instantiations (7 x 4); it is a condition, not a measurement.
 *
 * tpe_joint_wide_mixed_args starts with the fields of tpe_joint_wide_args at
 * the same offsets (low / high beyond n_dims are not read).  n_cat = 0 is
 * tpe_joint_wide_run on those fields.  Narrow groups are accepted so that the
 * stage can be compared with tpe_joint_mixed_run.  Returns TPE_E_ARG before any
 * launch (no device needed), checked in this order, for: null args; n_cat
 * outside [0, TPE_JOINT_WIDE_MAX_CAT]; n_dims < 1 or n_dims + n_cat >
 * TPE_JOINT_WIDE_MAX_DIMS; everything tpe_joint_wide_run checks on the shared
 * fields; a null table; a U_d outside [2, TPE_JOINT_MAX_CATS]; more than
 * TPE_JOINT_MAX_CAT_TOTAL categories; a cat_off that leaves [0, total - U_d];
 * scratch smaller than tpe_joint_wide_mixed_scratch_bytes.  As in
 * tpe_joint_mixed_run an injected category outside its table is the caller's
 * error.  tpe_joint_run_shard does not take this stage (the kernels' argument
 * structs carry cand_base, always 0 here).  Advances the resident-level epoch
 * as the other stage runs do; tpe_joint_profile and tpe_joint_wide_profile (the
 * sampling kernel) serve it as they serve tpe_joint_wide_run.
 * ---------------------------------------------------------------------- */
#define TPE_JOINT_WIDE_MAX_CAT 8        /* discrete labels of a wide group */
typedef struct tpe_joint_wide_mixed_args {
  int32_t n_dims, n_cand, n_ids, flags;   /* as tpe_joint_wide_args; n_dims: the continuous labels */
  int32_t k_below, k_above;
  uint32_t stream_word;
  int32_t reserved;
  uint64_t seed;
  const float *below_mu, *below_a, *below_c;
  const float *above_mu, *above_a, *above_c;
  double below_base, above_base;
  const double* samp_cum;
  const float* samp;
  const int64_t* ids;
  const float* inject;                    /* device [n_cand * (n_dims + n_cat)] */
  double low[TPE_JOINT_WIDE_MAX_DIMS], high[TPE_JOINT_WIDE_MAX_DIMS];
  int32_t n_cat;                          /* the discrete labels */
  int32_t cat_upper[TPE_JOINT_WIDE_MAX_CAT];  /* U_d */
  int32_t cat_off[TPE_JOINT_WIDE_MAX_CAT];    /* start of dimension d in the flat tables */
  const float *below_cat, *above_cat;     /* device [K * n_cat] */
  const float *below_miss, *below_bonus;  /* device [total] */
  const float *above_miss, *above_bonus;
  const double* below_h;                  /* device [n_cat] */
  const double* cat_cum;                  /* device [total] */
} tpe_joint_wide_mixed_args;

/* the chunk records and the candidate block of one tpe_joint_wide_mixed_run
 * (n_cat = 0: tpe_joint_wide_scratch_bytes) */
int tpe_joint_wide_mixed_scratch_bytes(int32_t n_ids, int32_t n_cand, int32_t n_dims, int32_t n_cat, uint64_t* bytes);

/* as tpe_joint_wide_run; cand: device f32 [n_ids * n_cand * (n_dims + n_cat)] */
int tpe_joint_wide_mixed_run(const tpe_joint_wide_mixed_args* args, tpe_joint_wide_record* records, float* cand,
                             double* l_out, double* g_out, void* scratch, uint64_t scratch_bytes, void* stream);

/* ------------------------------------------------------------------------
 * Quantised joint stage (tpe_joint.hip; additive to ABI 24): a group that also
 * holds n_quant quantised labels (quniform / qloguniform), 1 <= n_quant <=
 * TPE_JOINT_MAX_QUANT.  Kernel coordinate order: the n_dims continuous labels,
 * the n_cat discrete ones, then the quantised ones; a quantised coordinate
 * travels as its lattice index (f32 in `cand` / `inject`, double in
 * tpe_joint_record.z), like a category.  The first fields are those of
 * tpe_joint_mixed_args at the same offsets and mean the same (n_dims = 0 and
 * n_cat = 0 are allowed: an all-quantised group).
 *
 * Quantised dimension d is a continuous dimension observed through bins: its
 * lattice has V_d = quant_v[d] values and V_d + 1 strictly increasing edges
 * e_0 = low .. e_V = high in the fit coordinate, at quant_edge_off[d] in
 * `quant_edges` (f64, n_edges entries in all); the host-side copies of e_0 and
 * e_V are low[n_dims + d] and high[n_dims + d] (the sampler's f32 clip is made
 * from them).  A component with (mu, sigma)
 * gives lattice value i the mass
 *   P_kd(i) = [Phi((e_{i+1} - mu) / sigma) - Phi((e_i - mu) / sigma)] / mass_kd,
 *   mass_kd = Phi((e_V - mu) / sigma) - Phi((e_0 - mu) / sigma),
 * every Phi difference taken between the two smaller tails (lower tails left
 * of mu, upper tails right of it, 1 - upper - lower for the bin that holds mu);
 * a tail with |e - mu| / (sigma sqrt 2) > 26.5 (below 2^-1018, where float64
 * would go subnormal) counts as exactly 0.
 * The log2 of a component's term gains sum_d log2 P_kd(i_d); a quantised
 * dimension adds nothing to c.
 *
 * k_joint_qtable (one launch per side) evaluates T[d][i][k] = log2 P_kd(i) in
 * f64 from below_qmu / below_qsigma (above_..: f64 [K * n_quant], component k,
 * dimension d at [k * n_quant + d]) and stores it as f32 in `quant_table`, a
 * caller-owned device workspace of tpe_joint_quant_table_bytes(k_below,
 * k_above, sum_d V_d) bytes: the below side's [sum V][K_below] (per lattice
 * value a contiguous run over k, dimensions in order), then the above side's.
 * An entry below TPE_JOINT_QFLOOR (a far bin's f64 mass is exactly 0: -inf
 * included) is stored as TPE_JOINT_QFLOOR; next to the prior row's term such a
 * term is 0 in f32.  The chunk kernel stages the table through LDS in component
 * tiles laid out [lattice value][component]; per (candidate, component,
 * quantised dimension) it costs one LDS read at the candidate's own lattice
 * index and one add.
 *
 * Sampling: word 0 picks the component and word 1 + j serves kernel coordinate
 * j, as in the other two stages (so the continuous and discrete coordinates are
 * those of a tpe_joint_mixed_run / tpe_joint_run over the group without its
 * quantised labels).  A quantised coordinate draws z exactly as a continuous
 * dimension with the sampler row quant_samp[(k * n_quant + d) * 5 ..] = {mu,
 * sigma, fa, fb, flip} would (clipped to [smallest float >= e_0, largest float
 * < e_V]); its lattice index is the number of interior edges e_1 .. e_{V-1}
 * that are <= (double) z.
 *
 * Limits (conditions that bound the instantiation set and the LDS tile, not
 * measurements): n_quant <= TPE_JOINT_MAX_QUANT, 2 <= V_d <=
 * TPE_JOINT_MAX_LATTICE, sum_d V_d <= TPE_JOINT_MAX_LATTICE_TOTAL, and beside a
 * quantised label n_dims <= 8 and n_cat <= 4.
 *
 * tpe_joint_quant_run returns TPE_E_ARG before any launch (no device needed)
 * for everything tpe_joint_mixed_run checks (with n_quant counted among the
 * coordinates), n_quant outside [0, TPE_JOINT_MAX_QUANT], n_dims > 8 or n_cat >
 * 4 while n_quant > 0, a V_d outside [2, TPE_JOINT_MAX_LATTICE], a total above
 * TPE_JOINT_MAX_LATTICE_TOTAL, a quant_edge_off that leaves [0, n_edges - V_d -
 * 1], a null edge / mu / sigma / sampler / table pointer, or a table workspace
 * smaller than tpe_joint_quant_table_bytes says.  n_quant = 0 is
 * tpe_joint_mixed_run on the shared fields: the same bytes.  With
 * TPE_JOINT_INJECT an out-of-range lattice index is the caller's error; the
 * device only keeps the table index in range.  tpe_joint_record,
 * tpe_joint_scratch_bytes and tpe_joint_profile serve this stage too;
 * tpe_joint_quant_profile reads the table kernels' time of a profiled run.
 * ---------------------------------------------------------------------- */
#define TPE_JOINT_MAX_QUANT 4            /* quantised labels per group */
#define TPE_JOINT_MAX_LATTICE 256        /* lattice values per quantised label */
#define TPE_JOINT_MAX_LATTICE_TOTAL 512  /* lattice values per group */
#define TPE_JOINT_QFLOOR (-4096.0f)      /* smallest stored log2 P_kd(i) */
typedef struct tpe_joint_quant_args {
  int32_t n_dims, n_cand, n_ids, flags;   /* as tpe_joint_mixed_args ... */
  int32_t k_below, k_above;
  uint32_t stream_word;
  int32_t n_cat;
  uint64_t seed;
  const float *below_mu, *below_a, *below_c;
  const float *above_mu, *above_a, *above_c;
  double below_base, above_base;
  const double* samp_cum;
  const float* samp;
  const int64_t* ids;
  const float* inject;                    /* device [n_cand * (n_dims + n_cat + n_quant)] */
  double low[TPE_JOINT_MAX_DIMS], high[TPE_JOINT_MAX_DIMS];
  int32_t cat_upper[TPE_JOINT_MAX_DIMS];
  int32_t cat_off[TPE_JOINT_MAX_DIMS];
  const float *below_cat, *above_cat;
  const float *below_miss, *below_bonus;
  const float *above_miss, *above_bonus;
  const double* below_h;
  const double* cat_cum;                  /* ... up to here */
  int32_t n_quant;                        /* the quantised labels */
  int32_t n_edges;                        /* entries of quant_edges */
  int32_t quant_v[TPE_JOINT_MAX_QUANT];         /* V_d */
  int32_t quant_edge_off[TPE_JOINT_MAX_QUANT];  /* e_0 of dimension d in quant_edges */
  const double* quant_edges;              /* device f64 [n_edges] */
  const double *below_qmu, *below_qsigma; /* device f64 [k_below * n_quant] */
  const double *above_qmu, *above_qsigma; /* device f64 [k_above * n_quant] */
  const float* quant_samp;                /* device f32 [k_below * n_quant * 5] */
  float* quant_table;                     /* device workspace */
  uint64_t quant_table_bytes;
} tpe_joint_quant_args;

int tpe_joint_quant_table_bytes(int32_t k_below, int32_t k_above, int32_t total_bins, uint64_t* bytes);

/* as tpe_joint_run; cand: device f32 [n_ids * n_cand * (n_dims + n_cat + n_quant)] */
int tpe_joint_quant_run(const tpe_joint_quant_args* args, tpe_joint_record* records, float* cand, double* l_out,
                        double* g_out, void* scratch, uint64_t scratch_bytes, void* stream);

/* Profiling only: while tpe_joint_profile is enabled a tpe_joint_quant_run also
 * times its two table launches together; *table_ms gets that device time of the
 * last such run (it WAITS for them). */
int tpe_joint_quant_profile(double* table_ms);

/* ------------------------------------------------------------------------
 * Wide quantised joint stage (tpe_joint.hip; additive to ABI 24): a group of
 * n_dims >= 1 continuous labels, 0 <= n_cat <= TPE_JOINT_WIDE_MAX_CAT discrete
 * ones and 1 <= n_quant <= TPE_JOINT_MAX_QUANT quantised ones, n_dims + n_cat +
 * n_quant <= TPE_JOINT_WIDE_MAX_DIMS.  Nothing is defined anew:
 *   model        that of the quantised joint stage above at a larger width: the
 *                lattice edges, P_kd(i), the table T[d][i][k] = log2 P_kd(i)
 *                built by the same k_joint_qtable launches into a workspace of
 *                tpe_joint_quant_table_bytes, the floor TPE_JOINT_QFLOOR; the
 *                discrete part that of the wide mixed stage.
 *   coordinates  the n_dims continuous labels, the n_cat discrete ones, then the
 *                n_quant quantised ones; a category and a lattice index travel
 *                as f32 in `cand` / `inject` and as double in
 *                tpe_joint_wide_record.z.  low / high [n_dims + d] are the outer
 *                edges of quantised dimension d, as in tpe_joint_quant_args.
 *   streams      word 0 of block 0 picks the component; word 1 + j serves kernel
 *                coordinate j, that is word (1 + j) & 3 of block (1 + j) >> 2.  A
 *                continuous coordinate is drawn as tpe_joint_wide_run draws it,
 *                a discrete one as tpe_joint_wide_mixed_run does, a quantised
 *                one as tpe_joint_quant_run does (the continuous draw through
 *                quant_samp, clipped in f32, then the number of interior edges
 *                <= (double) z by binary search).
 * So the continuous and discrete coordinates of a run equal those of a
 * tpe_joint_wide_mixed_run (n_cat = 0: tpe_joint_wide_run) over the group
 * without its quantised labels, and a run at a shape tpe_joint_quant_run also
 * takes draws that run's candidates, both bit for bit.
 *
 * Launches: k_joint_qtable once per side; k_joint_wide_quant_sample (skipped
 * under TPE_JOINT_INJECT) draws one candidate a thread into `scratch`, laid out
 * [256-candidate block][j][256] over all coordinates;
 * k_joint_wide_quant_chunk<DP, KP, QP, R> (DP the padded n_dims in {16, 24, 32,
 * 48, 64}, KP the padded n_cat in {0, 2, 8}, QP the padded n_quant in {1, 2, 4},
 * R = 2 candidates a lane for DP <= 32 and 1 above) scores a chunk of 256 R
 * candidates: rows, categories and the table stream through LDS in component
 * tiles of ONE length, the longest multiple of 8 (at most the wide stage's
 * tile) whose table tile [sum V + 1][tile + 4] f32 stays within 26 KiB, so that
 * a workgroup's LDS stays under 64 KiB; per (candidate, component, quantised
 * slot) one table read at the candidate's own lattice index and one add.
 * k_joint_wide_merge picks the winner.  No atomics: the same call twice gives
 * the same bytes.
 *
 * tpe_joint_wide_quant_args starts with the fields of tpe_joint_wide_mixed_args
 * at the same offsets; the quantised fields of tpe_joint_quant_args follow.
 * Returns TPE_E_ARG before any launch (no device needed) for: null args;
 * n_quant outside [1, TPE_JOINT_MAX_QUANT]; n_cat outside [0,
 * TPE_JOINT_WIDE_MAX_CAT]; n_dims < 1 or n_dims + n_cat + n_quant >
 * TPE_JOINT_WIDE_MAX_DIMS; everything tpe_joint_wide_run checks on the shared
 * fields; with n_cat > 0 everything tpe_joint_wide_mixed_run checks on the
 * category tables; everything tpe_joint_quant_run checks on the lattices, the
 * quantised rows and the table workspace; scratch smaller than
 * tpe_joint_wide_quant_scratch_bytes.  tpe_joint_run_shard does not take this
 * stage.  Advances the resident-level epoch as the other stage runs do;
 * tpe_joint_profile (scoring kernel, merge), tpe_joint_quant_profile (the table
 * launches) and tpe_joint_wide_quant_profile (the sampling kernel) serve it.
 * ---------------------------------------------------------------------- */
typedef struct tpe_joint_wide_quant_args {
  int32_t n_dims, n_cand, n_ids, flags;   /* as tpe_joint_wide_mixed_args ... */
  int32_t k_below, k_above;
  uint32_t stream_word;
  int32_t reserved;
  uint64_t seed;
  const float *below_mu, *below_a, *below_c;
  const float *above_mu, *above_a, *above_c;
  double below_base, above_base;
  const double* samp_cum;
  const float* samp;
  const int64_t* ids;
  const float* inject;                    /* device [n_cand * (n_dims + n_cat + n_quant)] */
  double low[TPE_JOINT_WIDE_MAX_DIMS], high[TPE_JOINT_WIDE_MAX_DIMS];
  int32_t n_cat;                          /* 0 allowed: the category tables may be NULL then */
  int32_t cat_upper[TPE_JOINT_WIDE_MAX_CAT];
  int32_t cat_off[TPE_JOINT_WIDE_MAX_CAT];
  const float *below_cat, *above_cat;
  const float *below_miss, *below_bonus;
  const float *above_miss, *above_bonus;
  const double* below_h;
  const double* cat_cum;                  /* ... up to here */
  int32_t n_quant;                        /* as tpe_joint_quant_args from here on */
  int32_t n_edges;
  int32_t quant_v[TPE_JOINT_MAX_QUANT];
  int32_t quant_edge_off[TPE_JOINT_MAX_QUANT];
  const double* quant_edges;
  const double *below_qmu, *below_qsigma;
  const double *above_qmu, *above_qsigma;
  const float* quant_samp;
  float* quant_table;
  uint64_t quant_table_bytes;
} tpe_joint_wide_quant_args;

/* the chunk records and the candidate block of one tpe_joint_wide_quant_run */
int tpe_joint_wide_quant_scratch_bytes(int32_t n_ids, int32_t n_cand, int32_t n_dims, int32_t n_cat, int32_t n_quant,
                                       uint64_t* bytes);

/* as tpe_joint_wide_run; cand: device f32 [n_ids * n_cand * (n_dims + n_cat + n_quant)] */
int tpe_joint_wide_quant_run(const tpe_joint_wide_quant_args* args, tpe_joint_wide_record* records, float* cand,
                             double* l_out, double* g_out, void* scratch, uint64_t scratch_bytes, void* stream);

/* Profiling only: the sampling kernel's time (ms) of the last profiled sampling
 * tpe_joint_wide_quant_run (it WAITS for it). */
int tpe_joint_wide_quant_profile(double* sample_ms);

/* ------------------------------------------------------------------------
 * Segmented joint stage (tpe_joint.hip; additive to ABI 24): one call scores the
 * (new id, group) problems of MANY continuous groups, each group ("segment")
 * with its own model, dimension count and Philox stream word.  It serves joint
 * TPE on conditional branches (DESIGN.md "Branch groups"): in a batched suggest
 * over a tree every id takes its own branch, so every id needs its branch's
 * model.  A group's rows are those of tpe_joint_args, laid side by side in two
 * pools; tpe_joint_seg says where:
 *   pool_f32   every group's mu / a / c rows of both sides, its sampler rows
 *              samp[k_below * n_dims * 5] and, under TPE_JOINT_INJECT, its
 *              candidates [n_cand * n_dims]; the descriptor fields are ELEMENT
 *              offsets of their first float
 *   pool_f64   every group's samp_cum[k_below]
 *   lo / hi    the f32 bounds tpe_joint_run derives from low / high, made by the
 *              caller: the smallest float >= low_d, the largest float < high_d,
 *              -inf / +inf where unbounded and for d >= n_dims
 * Problem p = (prob_id[p], segment prob_seg[p]).
 *
 * Defining property: the record, the cand rows, l_out and g_out of problem p
 * are byte for byte those of a tpe_joint_run over that segment's rows with its
 * stream_word, ids = [prob_id[p]] and the same seed, n_cand and flags; the order
 * of the problems does not matter.  The device code is tpe_joint_run's:
 * k_joint_seg_chunk<DP> (one 256-thread workgroup per problem and chunk of
 * TPE_JOINT_CHUNK candidates) reads its problem's descriptor into scalar
 * registers and runs k_joint_chunk's body; k_joint_merge then picks every
 * problem's winner.  Launches, all on `stream` with no sync between them:
 * k_joint_seg_order (ranks the problems by DP class, then segment, then index,
 * into `scratch`: consecutive workgroups share a model), one k_joint_seg_chunk
 * launch per DP class present (1, 2, 3, 4, 6, 8, 12, 16), one k_joint_merge over
 * all problems.  Plain vector stores, no atomics: the same call twice gives the
 * same bytes.
 *
 * tpe_joint_seg_run returns TPE_E_ARG before any launch (no device needed) for
 * null args / segs / pools / problem arrays / records, n_segs < 1, n_probs < 1,
 * n_cand < 1, a host_prob_seg entry outside [0, n_segs), a host_segs entry with
 * n_dims outside [1, TPE_JOINT_MAX_DIMS], k_below < 1, k_above < 1 or rows that
 * leave its pool (pool_f32_len / pool_f64_len elements), TPE_JOINT_INJECT with a
 * problem whose segment has no candidates (inject < 0), cand without cand_off,
 * or scratch smaller than tpe_joint_seg_scratch_bytes(n_probs, n_cand).
 * host_segs / host_prob_seg are the caller's host copies of segs / prob_seg
 * (the checks and the launch sizes read them; the kernels read the device
 * arrays).  A segment with no problem is legal.  tpe_joint_profile covers this
 * stage: {the launches before the merge, summed; the merge}.
 * ---------------------------------------------------------------------- */
typedef struct tpe_joint_seg {
  int32_t n_dims, k_below, k_above;
  uint32_t stream_word;
  double below_base, above_base;
  int64_t below_mu, below_a, below_c;     /* element offsets in pool_f32 */
  int64_t above_mu, above_a, above_c;
  int64_t samp;
  int64_t inject;                         /* TPE_JOINT_INJECT: [n_cand * n_dims]; < 0: none */
  int64_t samp_cum;                       /* element offset in pool_f64 */
  float lo[TPE_JOINT_MAX_DIMS], hi[TPE_JOINT_MAX_DIMS];
} tpe_joint_seg;
typedef struct tpe_joint_seg_args {
  int32_t n_segs, n_probs, n_cand, flags;   /* flags: TPE_JOINT_INJECT */
  uint64_t seed;
  const tpe_joint_seg* segs;        /* device [n_segs] */
  const tpe_joint_seg* host_segs;   /* host   [n_segs], the same bytes */
  const float* pool_f32;            /* device */
  const double* pool_f64;           /* device (may be NULL under TPE_JOINT_INJECT) */
  int64_t pool_f32_len, pool_f64_len;   /* elements */
  const int32_t* prob_seg;          /* device [n_probs] */
  const int32_t* host_prob_seg;     /* host   [n_probs], the same bytes */
  const int64_t* prob_id;           /* device [n_probs] */
  const int64_t* cand_off;          /* device [n_probs]: element offset of problem p's rows in `cand` (NULL without cand) */
} tpe_joint_seg_args;

/* the problem order and the chunk records of one tpe_joint_seg_run */
int tpe_joint_seg_scratch_bytes(int32_t n_probs, int32_t n_cand, uint64_t* bytes);

/* records: device [n_probs], in the caller's problem order; optional (NULL: not
 * written) cand: device f32, problem p's [n_cand * n_dims(p)] rows from
 * cand_off[p] on; l_out / g_out: device f64 [n_probs * n_cand]; enqueued on
 * `stream` */
int tpe_joint_seg_run(const tpe_joint_seg_args* args, tpe_joint_record* records, float* cand, double* l_out,
                      double* g_out, void* scratch, uint64_t scratch_bytes, void* stream);

/* ------------------------------------------------------------------------
 * Wide segmented joint stage (tpe_joint.hip; additive to ABI 24): the segmented
 * stage for continuous groups of up to TPE_JOINT_WIDE_MAX_DIMS labels (DESIGN.md
 * "Wide branch groups").  tpe_joint_wide_seg is tpe_joint_seg with 64 f32 bounds
 * and n_dims in [1, TPE_JOINT_WIDE_MAX_DIMS]; the pools, the problems and the
 * args are tpe_joint_seg_args'; the records are tpe_joint_wide_record.
 *
 * Defining property: the record, the cand rows, l_out and g_out of problem p =
 * (prob_id[p], segment prob_seg[p]) are byte for byte those of a
 * tpe_joint_wide_run over that segment's rows with its stream_word, ids =
 * [prob_id[p]] and the same seed, n_cand and flags, with and without
 * TPE_JOINT_INJECT; the order of the problems does not matter.  The device code
 * is tpe_joint_wide_run's: the kernels below read their problem's descriptor
 * into scalar registers, build the solo kernels' argument view from it and run
 * the solo kernels' parts (the sampler steps, wide_load, score_side_wide,
 * wide_finish).  Launches, all on `stream` with no sync between them:
 * k_joint_seg_order over the wide classes (ranks the problems by DP class 20,
 * 24, 32, 48, 64, then segment, then index); k_joint_wide_seg_sample (skipped
 * under TPE_JOINT_INJECT; one workgroup per problem and block of 256 candidates,
 * the block's [d][256] floats written to the problem's slab of `scratch`; a
 * slab is [blocks][n_dims][256] and slabs are TPE_JOINT_WIDE_MAX_DIMS wide
 * apart); one k_joint_wide_seg_chunk<DP, R> launch per DP class present (one
 * workgroup per problem of the class and chunk of 256 R candidates, R = 2 for DP
 * <= 32 and 1 above); k_joint_wide_merge over all problems.  The chunk records
 * of a problem are ceil(n_cand / 256) apart, the count at R = 1; an R = 2
 * workgroup marks the slot behind its class's count as empty (global_idx = -1),
 * so the merge reads one stride.  Plain vector stores, no atomics: the same
 * call twice gives the same bytes.
 *
 * tpe_joint_wide_seg_run returns TPE_E_ARG before any launch (no device needed)
 * for everything tpe_joint_seg_run checks, with n_dims outside [1,
 * TPE_JOINT_WIDE_MAX_DIMS] in place of its range and scratch smaller than
 * tpe_joint_wide_seg_scratch_bytes(n_probs, n_cand).  A segment with no problem
 * is legal.  tpe_joint_profile covers this stage as it covers tpe_joint_seg_run
 * (the order kernel and the chunk launches, summed; the merge), and
 * tpe_joint_wide_profile reads its sampling kernel's time.
 * ---------------------------------------------------------------------- */
typedef struct tpe_joint_wide_seg {
  int32_t n_dims, k_below, k_above;       /* as tpe_joint_seg ... */
  uint32_t stream_word;
  double below_base, above_base;
  int64_t below_mu, below_a, below_c;
  int64_t above_mu, above_a, above_c;
  int64_t samp;
  int64_t inject;
  int64_t samp_cum;
  float lo[TPE_JOINT_WIDE_MAX_DIMS], hi[TPE_JOINT_WIDE_MAX_DIMS];   /* ... with 64 bounds */
} tpe_joint_wide_seg;
typedef struct tpe_joint_wide_seg_args {
  int32_t n_segs, n_probs, n_cand, flags;   /* as tpe_joint_seg_args */
  uint64_t seed;
  const tpe_joint_wide_seg* segs;
  const tpe_joint_wide_seg* host_segs;
  const float* pool_f32;
  const double* pool_f64;
  int64_t pool_f32_len, pool_f64_len;
  const int32_t* prob_seg;
  const int32_t* host_prob_seg;
  const int64_t* prob_id;
  const int64_t* cand_off;
} tpe_joint_wide_seg_args;

/* the problem order, the chunk records and the candidate slabs of one
 * tpe_joint_wide_seg_run (sized for 64 coordinates a problem) */
int tpe_joint_wide_seg_scratch_bytes(int32_t n_probs, int32_t n_cand, uint64_t* bytes);

/* as tpe_joint_seg_run, with tpe_joint_wide_record records */
int tpe_joint_wide_seg_run(const tpe_joint_wide_seg_args* args, tpe_joint_wide_record* records, float* cand,
                           double* l_out, double* g_out, void* scratch, uint64_t scratch_bytes, void* stream);

/* ------------------------------------------------------------------------
 * Mixed segmented joint stage (tpe_joint.hip; additive to ABI 24): the
 * segmented stage for groups that may also hold discrete and quantised labels
 * (DESIGN.md "Discrete and quantised labels in branch groups").  A segment is
 * a group of tpe_joint_quant_args' kind: n_dims continuous, n_cat discrete and
 * n_quant quantised coordinates in that kernel order.  tpe_joint_mseg starts
 * with the fields of tpe_joint_seg at the same offsets (n_dims counts the
 * continuous coordinates; `inject` rows are [n_cand * (n_dims + n_cat +
 * n_quant)]) and then says, as ELEMENT offsets, where the rest of what
 * tpe_joint_quant_args carries per group lies:
 *   pool_f32   below_cat / above_cat [K * n_cat], below_miss / below_bonus /
 *              above_miss / above_bonus [sum U_d], quant_samp [k_below *
 *              n_quant * 5] (and, as in tpe_joint_seg, the mu / a / c rows, samp
 *              and the injected rows)
 *   pool_f64   below_h [n_cat], cat_cum [sum U_d], quant_edges [n_edges],
 *              below_qmu / below_qsigma [k_below * n_quant], above_qmu /
 *              above_qsigma [k_above * n_quant] (and samp_cum)
 *   cat_upper / cat_off, quant_v / quant_edge_off   as in tpe_joint_quant_args
 *   lo / hi, qlo / qhi   the f32 clip bounds of the continuous and the quantised
 *              coordinates (the smallest float >= e_0, the largest float < e_V)
 *   table      the element offset of the segment's table in `quant_table`, one
 *              caller-owned device workspace of f32: the below side's [sum V]
 *              [k_below], then the above side's, (k_below + k_above) sum V
 *              elements; tpe_joint_mseg_table_bytes gives the bytes of all
 *              segments laid end to end in descriptor order
 *
 * Defining property: the record, the cand rows, l_out and g_out of problem p are
 * byte for byte those of a solo run over its segment alone with the segment's
 * stream_word, ids = [prob_id[p]] and the same seed, n_cand and flags:
 * tpe_joint_quant_run when n_quant > 0, tpe_joint_mixed_run when n_quant = 0 and
 * n_cat > 0, tpe_joint_run when both are 0.  The order of the problems does not
 * matter; the same call twice gives the same bytes (plain vector stores, no
 * atomics).  The device code is the solo stages': their chunk bodies are
 * __device__ functions that both kinds of kernel call.
 *
 * Launches, all on `stream` with no sync between them: k_joint_seg_order (ranks
 * the problems by kernel class (CP, KP, QP), then segment, then index; the
 * continuous DP classes are the first eight), k_joint_mseg_qtable (one launch:
 * T[d][i][k] of every quantised segment and side, k_joint_qtable's arithmetic
 * and TPE_JOINT_QFLOOR), one chunk launch per class present —
 * k_joint_seg_chunk<DP>, k_joint_mseg_mixed_chunk<CP, KP> (CP in {0, 2, 4, 8},
 * KP in {1, 2, 4}) or k_joint_mseg_quant_chunk<CP, KP, QP> (the 48 shapes of
 * the solo stage) — and k_joint_merge over all problems.  A quantised segment's
 * LDS tile and row stride are derived from its own lattice total by the solo
 * run's rule; a class launch takes the largest dynamic LDS among its segments.
 *
 * Limits (they bound the set of compiled kernels; they are not measurements):
 * a segment with n_cat + n_quant > 0 has n_dims <= 8, n_cat <= 4, n_quant <=
 * TPE_JOINT_MAX_QUANT, and the category and lattice limits of the solo stages; a
 * continuous segment has 1 <= n_dims <= TPE_JOINT_MAX_DIMS.
 *
 * tpe_joint_mseg_run returns TPE_E_ARG before any launch (no device needed) for
 * everything tpe_joint_seg_run checks and, per host descriptor, everything
 * tpe_joint_quant_run checks: counts outside their limits, n_dims > 8 or n_cat >
 * 4 beside a discrete or quantised coordinate, a U_d or V_d outside its range, a
 * category or lattice total above its limit, a cat_off or quant_edge_off outside
 * its tables, a null f64 pool or table workspace where a segment needs it, rows,
 * edges or a table that leave their pool or the workspace, more than 32767
 * segments, or scratch smaller than tpe_joint_mseg_scratch_bytes says.
 * tpe_joint_profile covers this stage as it covers tpe_joint_seg_run.
 * ---------------------------------------------------------------------- */
#define TPE_JOINT_MSEG_MAX_CONT 8   /* continuous coordinates beside a discrete / quantised one */
#define TPE_JOINT_MSEG_MAX_CAT 4    /* discrete coordinates of a segment */
typedef struct tpe_joint_mseg {
  int32_t n_dims, k_below, k_above;       /* as tpe_joint_seg ... */
  uint32_t stream_word;
  double below_base, above_base;
  int64_t below_mu, below_a, below_c;
  int64_t above_mu, above_a, above_c;
  int64_t samp;
  int64_t inject;
  int64_t samp_cum;
  float lo[TPE_JOINT_MAX_DIMS], hi[TPE_JOINT_MAX_DIMS];   /* ... up to here */
  int32_t n_cat, n_quant;
  int32_t cat_upper[TPE_JOINT_MSEG_MAX_CAT], cat_off[TPE_JOINT_MSEG_MAX_CAT];
  int32_t quant_v[TPE_JOINT_MAX_QUANT], quant_edge_off[TPE_JOINT_MAX_QUANT];
  float qlo[TPE_JOINT_MAX_QUANT], qhi[TPE_JOINT_MAX_QUANT];
  int32_t n_edges, reserved;
  int64_t below_cat, above_cat;           /* element offsets in pool_f32 */
  int64_t below_miss, below_bonus, above_miss, above_bonus;
  int64_t quant_samp;
  int64_t below_h, cat_cum;               /* element offsets in pool_f64 */
  int64_t quant_edges;
  int64_t below_qmu, below_qsigma, above_qmu, above_qsigma;
  int64_t table;                          /* element offset in quant_table */
} tpe_joint_mseg;
typedef struct tpe_joint_mseg_args {
  int32_t n_segs, n_probs, n_cand, flags;   /* as tpe_joint_seg_args ... */
  uint64_t seed;
  const tpe_joint_mseg* segs;
  const tpe_joint_mseg* host_segs;
  const float* pool_f32;
  const double* pool_f64;
  int64_t pool_f32_len, pool_f64_len;
  const int32_t* prob_seg;
  const int32_t* host_prob_seg;
  const int64_t* prob_id;
  const int64_t* cand_off;                  /* ... up to here */
  float* quant_table;                       /* device workspace (may be NULL without a quantised segment) */
  uint64_t quant_table_bytes;
} tpe_joint_mseg_args;

/* the problem order and the chunk records of one tpe_joint_mseg_run */
int tpe_joint_mseg_scratch_bytes(int32_t n_probs, int32_t n_cand, uint64_t* bytes);

/* the table workspace of the host descriptors: sum over the segments with
 * n_quant > 0 of (k_below + k_above) * sum_d V_d floats */
int tpe_joint_mseg_table_bytes(const tpe_joint_mseg* host_segs, int32_t n_segs, uint64_t* bytes);

/* as tpe_joint_seg_run; problem p's cand rows are [n_cand * (n_dims + n_cat +
 * n_quant)(p)], categories and lattice indices as f32 */
int tpe_joint_mseg_run(const tpe_joint_mseg_args* args, tpe_joint_record* records, float* cand, double* l_out,
                       double* g_out, void* scratch, uint64_t scratch_bytes, void* stream);

/* ------------------------------------------------------------------------
 * Sharded joint stage (additive export; the ABI stays 24).  Any of the six
 * joint stages over the candidates [cand_base, cand_base + n_cand) of a run of
 * n_cand_global candidates: a rank's share of a candidate-sharded joint
 * suggest (tpe.suggest(..., joint_shard=(rank, world))).
 *
 * `stage` names the entry point whose `args` and record type the call takes
 * (TPE_JOINT_STAGE_*).  args->n_cand is the LOCAL count; local candidate i is
 * global candidate g = cand_base + i.  The first Philox counter word of every
 * draw is g (everything else about the draws as the stage documents it), and
 * record.global_idx is g.  cand, l_out and g_out are local arrays indexed by
 * i, and scratch (and the table workspace) are sized by the stage's own
 * *_scratch_bytes / *_table_bytes at the local n_cand.  A candidate is a
 * function of (seed, stream word, new id, g) alone and a record's order key of
 * (score, g), so the records of the parts of a partition, combined in
 * np.argmax order (NaN first, the larger l - g, the lower global_idx; an empty
 * record, global_idx < 0, never wins), are the bytes of the unsharded run.
 * The six stage entry points are this call with shard {0, n_cand}.
 *
 * Returns TPE_E_ARG before any launch (no device needed) for null args or
 * shard, a stage outside [0, 5], cand_base < 0, cand_base + n_cand >
 * n_cand_global, n_cand_global >= 2^31 (the counter word and the index
 * arithmetic are 32-bit), TPE_JOINT_INJECT with cand_base != 0 (injected rows
 * have no global index), and for everything the stage's own entry point
 * rejects.  Advances the resident-level epoch as the stage runs do.
 * ---------------------------------------------------------------------- */
#define TPE_JOINT_STAGE_RUN 0   /* args: tpe_joint_args,       records: tpe_joint_record      */
#define TPE_JOINT_STAGE_WIDE 1  /*       tpe_joint_wide_args,           tpe_joint_wide_record */
#define TPE_JOINT_STAGE_MIXED 2 /*       tpe_joint_mixed_args,          tpe_joint_record      */
#define TPE_JOINT_STAGE_QUANT 3 /*       tpe_joint_quant_args                                 */
#define TPE_JOINT_STAGE_SEG 4   /*       tpe_joint_seg_args                                   */
#define TPE_JOINT_STAGE_MSEG 5  /*       tpe_joint_mseg_args                                  */
typedef struct tpe_joint_shard {
  int64_t cand_base, n_cand_global;
} tpe_joint_shard;
int tpe_joint_run_shard(int32_t stage, const void* args, const tpe_joint_shard* shard, void* records, float* cand,
                        double* l_out, double* g_out, void* scratch, uint64_t scratch_bytes, void* stream);

/* ------------------------------------------------------------------------
 * Batch-aware joint suggests (tpe_joint_liar.hip, which also holds the stage
 * for discrete and quantised labels below; additive exports, the ABI stays
 * 24).  A follow-up stage of tpe_joint_run / tpe_joint_wide_run, enqueued
 * after the stage that wrote cand, l_out and g_out (as tpe_joint_report is):
 * the ids pick greedily, in the order given.  Id 0 picks as the stage itself
 * does; its vector then joins the above mixture as one more component, a
 * "liar" (a point not yet evaluated, counted as bad), id 1 picks under that
 * mixture, and so on.  n_given vectors may be liars before step 0; i is a
 * liar's ordinal among all liars, the given ones first.
 *
 * The above side has n = n_trials trial rows and the prior row (k_above rows of
 * above_mu, the f32 rows as uploaded), un-normalised weights w~ with W = w_sum
 * their sum.  Liar i has un-normalised weight 1 and mean mu = z, the f32
 * coordinates of the pick (or given vector).  Its bandwidth in dimension d is
 * the adaptive-Parzen neighbour rule over P_d = the k_above values
 * above_mu[., d] and the z_d of the liars before it: L = max{p in P_d: p <=
 * z_d}, U = min{p in P_d: p > z_d}, sigma = max(z_d - L, U - z_d) (a missing
 * side is dropped; none: 0), clipped to [psig_d / min(100, m + 2), psig_d] with
 * m = n + i + 1: float64 arithmetic on f32 values, so liar_sigma is the same
 * bits on every IEEE machine.  The existing components keep their bandwidths.
 *
 * With J = n_given + j liars, step j scores
 *   log g_j(z) = logaddexp(log g(z), logsumexp_i log k_i(z) - log W) - log1p(J / W)
 *   log k_i(z) = - sum_d [ log(sigma_id sqrt(2 pi) mass_id) + ((z_d - mu_id) / sigma_id)^2 / 2 ]
 * (mass: of the normal truncated to [low_d, high_d), 1 where unbounded), the
 * liar term in float64; score_j = l - g_j, l and g read from l_out / g_out of
 * id j; winner in np.argmax order (NaN first, ties to the lower index).  With
 * J = 0, g_0 = g: pick 0 is the stage's own record.
 *
 * Outputs: picks[j] = {candidate index, l, g_j}; pick_z[j * n_dims ..] the
 * winner's row, copied bit for bit; liar_sigma[i * n_dims ..] for every liar
 * (the last pick's too).  2 launches a step (k_liar_pick<false>, one workgroup,
 * and k_liar_chunk<false>, TPE_JOINT_CHUNK candidates a workgroup; liar rows
 * stream through LDS in tiles of TPE_JOINT_LIAR_TILE), ordered by the stream
 * alone.
 * No atomics: the same call twice gives the same bytes.
 *
 * tpe_joint_liar_scratch_bytes = (n_given + n_ids) (2 n_dims + 1) 8 +
 * ceil(n_cand / TPE_JOINT_CHUNK) 24.  tpe_joint_liar returns TPE_E_ARG before
 * any launch (no device needed) for null args, buffers or outputs, n_dims
 * outside [1, TPE_JOINT_WIDE_MAX_DIMS], n_ids, n_cand or k_above < 1, n_given
 * or n_trials < 0, n_given > 0 without `given`, w_sum not positive and finite,
 * a psig that is not positive, or scratch smaller than that.
 * ---------------------------------------------------------------------- */
#define TPE_JOINT_LIAR_TILE 32
typedef struct tpe_joint_pick {
  int64_t idx;                 /* the winner's candidate index in its id's pool */
  double l, g;                 /* g: log g_j at the winner */
} tpe_joint_pick;
typedef struct tpe_joint_liar_args {
  int32_t n_dims, n_cand, n_ids, n_given;
  int32_t k_above, n_trials;
  double w_sum;
  const float* cand;           /* device [n_ids * n_cand * n_dims] */
  const double *l_out, *g_out; /* device [n_ids * n_cand] */
  const float* above_mu;       /* device [k_above * n_dims] */
  const float* given;          /* device [n_given * n_dims]; NULL with n_given == 0 */
  double psig[TPE_JOINT_WIDE_MAX_DIMS];                                    /* the prior sigmas */
  double low[TPE_JOINT_WIDE_MAX_DIMS], high[TPE_JOINT_WIDE_MAX_DIMS];      /* -inf / +inf: unbounded */
} tpe_joint_liar_args;

int tpe_joint_liar_scratch_bytes(int32_t n_ids, int32_t n_cand, int32_t n_dims, int32_t n_given, uint64_t* bytes);

/* picks: device [n_ids]; pick_z: device f32 [n_ids * n_dims]; liar_sigma:
 * device f64 [(n_given + n_ids) * n_dims]; enqueued on `stream` */
int tpe_joint_liar(const tpe_joint_liar_args* args, tpe_joint_pick* picks, float* pick_z, double* liar_sigma,
                   void* scratch, uint64_t scratch_bytes, void* stream);

/* ------------------------------------------------------------------------
 * Batch-aware picks over discrete and quantised labels
 * (tpe_joint_liar.hip, the <true> instantiations of its two kernel templates;
 * additive exports, the ABI stays 24).  The liar
 * stage above for a group that also holds n_cat discrete and / or n_quant
 * quantised labels: a follow-up of tpe_joint_mixed_run, tpe_joint_wide_mixed_run
 * or tpe_joint_quant_run, enqueued after the stage that wrote cand, l_out and
 * g_out.  A row (of `cand`, `given`, pick_z) is [z (f32, n_dims) | category
 * index (n_cat) | lattice index (n_quant)], D = n_dims + n_cat + n_quant wide.
 * Steps, ordering, W, m = n + i + 1, the score, the winner order and the
 * outputs are tpe_joint_liar's; the existing components are not refitted, their
 * smoothing masses included.  Liar i at a row r:
 *   continuous d < n_dims   tpe_joint_liar's rule over above_mu[., d] (f32) and
 *                           the earlier liars' coordinates.
 *   discrete d              the category x = r[n_dims + d] and the factor of a
 *                           trial component of the above side as the stage holds
 *                           it, P(v) = (1[v = x] + s_d p_d(v)) / (1 + s_d), from
 *                           the f64 tables cat_miss[cat_off[d] + v] = ln(s_d
 *                           p_d(v) / (1 + s_d)) and cat_bonus[..] = ln(1 + 1 /
 *                           (s_d p_d(v))) (natural logarithms); no bandwidth.
 *   quantised d             centre c = quant_centre[t_d + v], v = r[n_dims +
 *                           n_cat + d], t_d = sum of V_e over e < d: the fit
 *                           coordinate of the picked lattice value, a host table
 *                           the device only indexes.  Bandwidth: the neighbour
 *                           rule over the k_above values above_qmu[., d] (f64,
 *                           the prior row included) and the centres of the liars
 *                           before it, L = max{p <= c}, U = min{p > c}, sigma =
 *                           max(c - L, U - c) (a missing side dropped; none: 0),
 *                           clipped to [psig / min(100, m + 2), psig] with psig
 *                           = psig[n_dims + d]: f64 subtractions, one division,
 *                           max / min, so the same bits on every IEEE machine.
 *                           Factor Q_i(v): the normal (c, sigma) on the bin
 *                           [e_v, e_v+1) over its mass on [e_0, e_V), by the
 *                           quantised stage's rule (differences between the two
 *                           smaller tails, a tail beyond 26.5 exactly 0), in f64
 *                           and NOT floored: a far bin's log is -inf and the
 *                           liar adds exactly 0 there.
 *   log k_i(z, v, q) = tpe_joint_liar's continuous term + sum_d ln P_id(v_d) +
 *                      sum_d ln Q_id(q_d)
 *   log g_j = logaddexp(log g, logsumexp_i log k_i - log W) - log1p(J / W);
 * where every liar's term is -inf, g_j = log g - log1p(J / W), no NaN.
 *
 * Outputs: picks[j] as tpe_joint_liar; pick_z[j * D ..] the winner's row, bit
 * for bit; liar_sigma[i * (n_dims + n_quant) ..]: the continuous dimensions,
 * then the quantised ones, for every liar (the last pick's too).  2 launches a
 * step: k_liar_pick<true> (one workgroup: merge, row copy, the two neighbour
 * sweeps, then the liar's tables T_i[d][v] = ln Q_i(v), one thread per lattice
 * value, the V_d + 1 tails once through LDS) and k_liar_chunk<true>
 * (TPE_JOINT_CHUNK candidates a workgroup, four a lane; liar rows {mu, sqrt(1/2)
 * / sigma, c, category, centre} through LDS in tiles of TPE_JOINT_LIAR_TILE;
 * per (candidate, liar) one compare-select-add per discrete dimension and one
 * table read through L1 / L2 at the candidate's own lattice index per quantised
 * one; sum_d miss_d(v_d) after the sum over the liars).  Ordered by the stream
 * alone, no atomics: the same call twice gives the same bytes.  As in the base
 * stages a category or lattice index outside its table is the caller's error;
 * the device only keeps its table indices in range.
 *
 * tpe_joint_liar_mixed_scratch_bytes = (n_given + n_ids) (2 n_dims + 1 + n_cat
 * + n_quant + n_lattice) 8 + ceil(n_cand / TPE_JOINT_CHUNK) 24, n_lattice = sum_d
 * V_d; TPE_E_ARG for counts out of range.  tpe_joint_liar_mixed_args starts with
 * the fields of tpe_joint_liar_args at the same offsets (n_dims: the continuous
 * labels; low / high [n_dims + d] are not read).  With n_cat = n_quant = 0 the
 * call IS tpe_joint_liar on that prefix: its checks, its bytes.  Otherwise
 * tpe_joint_liar_mixed returns TPE_E_ARG before any launch (no device needed)
 * for: null args, buffers or outputs (above_mu may be NULL with n_dims = 0); a
 * negative count; n_cat > TPE_JOINT_MAX_DIMS, n_quant > TPE_JOINT_MAX_QUANT; D
 * outside [1, TPE_JOINT_WIDE_MAX_DIMS]; n_dims > 8 or n_cat > 4 while n_quant >
 * 0; n_ids, n_cand or k_above < 1; n_given > 0 without `given`; w_sum not
 * positive and finite; a psig (continuous or quantised) that is not positive; a
 * null table while its count is > 0; a U_d outside [2, TPE_JOINT_MAX_CATS], more
 * than TPE_JOINT_MAX_CAT_TOTAL categories, a cat_off that leaves [0, total -
 * U_d]; a V_d outside [2, TPE_JOINT_MAX_LATTICE], more than
 * TPE_JOINT_MAX_LATTICE_TOTAL lattice values, a quant_edge_off that leaves [0,
 * n_edges - V_d - 1]; scratch smaller than the formula.
 * ---------------------------------------------------------------------- */
typedef struct tpe_joint_liar_mixed_args {
  int32_t n_dims, n_cand, n_ids, n_given;  /* as tpe_joint_liar_args ...; n_dims: the continuous labels */
  int32_t k_above, n_trials;
  double w_sum;
  const float* cand;           /* device [n_ids * n_cand * D] */
  const double *l_out, *g_out; /* device [n_ids * n_cand] */
  const float* above_mu;       /* device [k_above * n_dims] */
  const float* given;          /* device [n_given * D]; NULL with n_given == 0 */
  double psig[TPE_JOINT_WIDE_MAX_DIMS];      /* [d] continuous, [n_dims + d] quantised dimension d */
  double low[TPE_JOINT_WIDE_MAX_DIMS], high[TPE_JOINT_WIDE_MAX_DIMS];   /* ... up to here; the continuous bounds */
  int32_t n_cat, n_quant;
  int32_t cat_upper[TPE_JOINT_MAX_DIMS];   /* U_d */
  int32_t cat_off[TPE_JOINT_MAX_DIMS];     /* start of dimension d in cat_miss / cat_bonus */
  const double *cat_miss, *cat_bonus;      /* device f64 [sum_d U_d], natural logarithms, the above side's s_d */
  int32_t quant_v[TPE_JOINT_MAX_QUANT];         /* V_d */
  int32_t quant_edge_off[TPE_JOINT_MAX_QUANT];  /* e_0 of dimension d in quant_edges */
  int32_t n_edges, reserved;
  const double* quant_edges;   /* device f64 [n_edges], as tpe_joint_quant_args */
  const double* quant_centre;  /* device f64 [sum_d V_d], dimensions in order */
  const double* above_qmu;     /* device f64 [k_above * n_quant], as tpe_joint_quant_args */
} tpe_joint_liar_mixed_args;

int tpe_joint_liar_mixed_scratch_bytes(int32_t n_ids, int32_t n_cand, int32_t n_dims, int32_t n_cat, int32_t n_quant,
                                       int32_t n_lattice, int32_t n_given, uint64_t* bytes);

/* picks: device [n_ids]; pick_z: device f32 [n_ids * D]; liar_sigma: device f64
 * [(n_given + n_ids) * (n_dims + n_quant)]; enqueued on `stream` */
int tpe_joint_liar_mixed(const tpe_joint_liar_mixed_args* args, tpe_joint_pick* picks, float* pick_z,
                         double* liar_sigma, void* scratch, uint64_t scratch_bytes, void* stream);

/* ------------------------------------------------------------------------
 * Batch-aware picks in branch groups (tpe_joint_liar.hip, k_liar_seg_chunk and
 * k_liar_seg_pick; additive exports, the ABI stays 24).  The liar stage for
 * the problems of a tpe_joint_seg_run: a follow-up enqueued on the same stream
 * over the cand / cand_off, l_out / g_out and pool_f32 that call just used.
 * Problem p = (prob_id[p], group prob_seg[p]).  The chain of group s is its
 * problems in the caller's order, step j its (j + 1)-th problem; chains of
 * different groups do not see each other, and there are no given liars.  Inside
 * a chain the model is tpe_joint_liar's with n_given = 0: liar weight 1, mean
 * the picked f32 row, the neighbour rule over the group's own above_mu rows
 * (pool_f32 + above_mu, k_above rows of n_dims) and the chain's earlier picks
 * with m = n_trials + j + 1, and log g_j = logaddexp(log g, lse - log W_s) -
 * log1p(j / W_s), W_s = w_sum.
 *
 * Defining property: picks, pick_z rows and liar_sigma rows of group s are byte
 * for byte those of a tpe_joint_liar with n_ids = chain_len over that group's
 * problems' cand, l_out and g_out in chain order, its above_mu, k_above,
 * n_trials, w_sum, psig, low, high and n_given = 0.  A chain of one problem is
 * tpe_joint_seg_run's record of that problem.  The device code is
 * tpe_joint_liar's: the bodies of k_liar_chunk<false> and k_liar_pick<false>
 * are device functions over a view of one group, which the segmented kernels
 * build from the group's descriptor in device memory.
 *
 * The caller orders the groups by chain length, longest first, ties by group
 * index (`order`: rank -> group), so the groups still active in round r are a
 * prefix.  `chain` lists the problems chain by chain in that order: group s
 * holds the slots [chain_first, chain_first + chain_len).  row_off / sigma_off
 * are the running sums, in the same order, of chain_len (2 n_dims + 1) and
 * chain_len n_dims: where the group's rows start in scratch and in liar_sigma,
 * in doubles.  log_w = log(w_sum) and log_norm[chain_first + j] = log1p(j /
 * w_sum) are the HOST C library's values, as tpe_joint_liar computes them (the
 * device's log differs in the last bits, and the bytes are the contract).
 *
 * Launches, all on `stream`, ordered by the stream alone: round r = 0 ..
 * (longest chain) - 1 runs k_liar_seg_chunk on a grid of (chunks of
 * TPE_JOINT_CHUNK candidates) x (groups with chain_len > r), then
 * k_liar_seg_pick with one 256-thread workgroup per such group: 2 x (longest
 * chain) launches.  No workgroup waits on another, no atomics, plain vector
 * stores, fixed reduction shapes: the same call twice gives the same bytes.
 *
 * tpe_joint_liar_seg_scratch_bytes = sum_s chain_len_s (2 n_dims_s + 1) 8 +
 * n_active ceil(n_cand / TPE_JOINT_CHUNK) 24, n_active the groups with
 * chain_len > 0; it reads n_dims and chain_len of host_segs and returns
 * TPE_E_ARG for null pointers, n_segs or n_cand < 1, an n_dims outside [1,
 * TPE_JOINT_MAX_DIMS] or a chain_len < 0.  tpe_joint_liar_seg returns TPE_E_ARG
 * before any launch (no device needed) for: null args, arrays or outputs;
 * n_segs, n_probs or n_cand < 1; a descriptor with n_dims outside [1,
 * TPE_JOINT_MAX_DIMS], k_above < 1, n_trials < 0, a w_sum that is not positive
 * and finite, a psig that is not positive, an above_mu range that leaves
 * pool_f32 (pool_f32_len elements) or a log_w that is not log(w_sum); a
 * host_prob_seg entry outside [0, n_segs); an order, chain_len, chain_first or
 * chain table that is not the partition of [0, n_probs) host_prob_seg gives; a
 * row_off or sigma_off that is not the running sum; a log_norm entry that is
 * not log1p(j / w_sum); more than 65535 groups with a problem; scratch smaller
 * than the formula.  The checks read the host copies; the kernels read the
 * device arrays, which must hold the same bytes.  cand_off is read on the
 * device alone, as by tpe_joint_seg_run.  A group without a problem is legal.
 * ---------------------------------------------------------------------- */
typedef struct tpe_joint_liar_seg_desc {
  int32_t n_dims, k_above, n_trials;
  int32_t chain_len;           /* L_s: the problems of this group */
  int32_t chain_first;         /* its first slot in `chain` */
  int32_t reserved;
  double w_sum, log_w;         /* W_s, log(W_s) by the host's C library */
  int64_t above_mu;            /* element offset in pool_f32, as tpe_joint_seg.above_mu */
  int64_t row_off, sigma_off;  /* doubles: the group's liar rows in scratch, its rows of liar_sigma */
  double psig[TPE_JOINT_MAX_DIMS];                                /* the prior sigmas */
  double low[TPE_JOINT_MAX_DIMS], high[TPE_JOINT_MAX_DIMS];       /* -inf / +inf: unbounded */
} tpe_joint_liar_seg_desc;
typedef struct tpe_joint_liar_seg_args {
  int32_t n_segs, n_probs, n_cand, reserved;
  const tpe_joint_liar_seg_desc* segs;        /* device [n_segs], group index order */
  const tpe_joint_liar_seg_desc* host_segs;   /* host   [n_segs], the same bytes */
  const int32_t* order;                  /* device [n_segs]: rank -> group */
  const int32_t* host_order;
  const int32_t* chain;                  /* device [n_probs]: slot -> problem */
  const int32_t* host_chain;
  const double* log_norm;                /* device [n_probs]: by slot */
  const double* host_log_norm;
  const int32_t* host_prob_seg;          /* host   [n_probs], as tpe_joint_seg_args */
  const float* cand;                     /* device, what tpe_joint_seg_run wrote */
  const int64_t* cand_off;               /* device [n_probs] */
  const double *l_out, *g_out;           /* device [n_probs * n_cand] */
  const float* pool_f32;                 /* device */
  int64_t pool_f32_len;                  /* elements */
} tpe_joint_liar_seg_args;

int tpe_joint_liar_seg_scratch_bytes(const tpe_joint_liar_seg_desc* host_segs, int32_t n_segs, int32_t n_cand,
                                     uint64_t* bytes);

/* picks: device [n_probs], by problem; pick_z: device f32 [n_probs *
 * TPE_JOINT_MAX_DIMS], problem p's row at p * TPE_JOINT_MAX_DIMS (n_dims
 * floats written); liar_sigma: device f64 [sum_s chain_len_s n_dims_s], group
 * s's [chain_len, n_dims] rows at sigma_off; enqueued on `stream` */
int tpe_joint_liar_seg(const tpe_joint_liar_seg_args* args, tpe_joint_pick* picks, float* pick_z,
                       double* liar_sigma, void* scratch, uint64_t scratch_bytes, void* stream);

/* ------------------------------------------------------------------------
 * Batch-aware picks in mixed branch groups (tpe_joint_liar.hip,
 * k_liar_mseg_chunk and k_liar_mseg_pick; additive exports, the ABI stays 24).
 * tpe_joint_liar_seg for the problems of a tpe_joint_mseg_run: a group may also
 * hold n_cat discrete and n_quant quantised labels.  Problems, chains, order,
 * slots, log_w and log_norm are tpe_joint_liar_seg's; there are no given liars.
 * Inside a chain the model is the solo stage of the group's kind with n_given =
 * 0: tpe_joint_liar_mixed's for a group with n_cat + n_quant > 0, tpe_joint_liar's
 * for a continuous one.  No new math.
 *
 * Defining property: picks, pick_z rows and liar_sigma rows of group s are byte
 * for byte those of a tpe_joint_liar_mixed (n_cat = n_quant = 0: tpe_joint_liar)
 * with n_ids = chain_len over that group's problems' cand, l_out and g_out in
 * chain order, its above_mu, above_qmu, tables, k_above, n_trials, w_sum, psig,
 * low, high and n_given = 0.  A chain of one problem is tpe_joint_mseg_run's
 * record of that problem.  The device code is tpe_joint_liar_mixed's: the bodies
 * of k_liar_chunk<true> and k_liar_pick<true> over a second view of one group,
 * built in registers from the group's descriptor in device memory, its
 * per-dimension arrays pointers into that descriptor.  A continuous group runs
 * the same bodies with n_cat = n_quant = 0, which gives k_liar_seg_*'s bytes.
 *
 * Descriptor: the fields of tpe_joint_liar_seg_desc at the same offsets (n_dims
 * counts the continuous labels; psig[n_dims + d] is quantised dimension d's),
 * then the group's discrete and quantised parts.  above_qmu [k_above * n_quant]
 * and quant_edges [n_edges] are ELEMENT offsets into the pool_f64 of the
 * tpe_joint_mseg_run before (the same values as in its tpe_joint_mseg).  cat_miss
 * / cat_bonus [sum U_d] (natural logarithms, as tpe_joint_liar_mixed_args) and
 * quant_centre [sum V_d] are element offsets into liar_pool, a device f64 array
 * of this call (liar_pool_len elements).  quant_tab_off[d] = sum of V_e over e <
 * d; n_lattice = sum V_d.  row_off, tab_off and sigma_off are the running sums,
 * in `order`, of chain_len (2 n_dims + 1 + n_cat + n_quant), chain_len n_lattice
 * and chain_len (n_dims + n_quant): the group's liar rows and liar bin tables
 * (ln Q_i(v), read through L1 / L2 as in the solo stage) in scratch, and its rows
 * of liar_sigma.
 *
 * Launches: tpe_joint_liar_seg's rounds with k_liar_mseg_chunk and
 * k_liar_mseg_pick: 2 x (longest chain) launches, ordered by the stream alone, no
 * atomics, plain vector stores, fixed reduction shapes: the same call twice
 * gives the same bytes.
 *
 * tpe_joint_liar_mseg_scratch_bytes = sum_s chain_len_s (2 n_dims + 1 + n_cat +
 * n_quant + n_lattice)_s 8 + n_active ceil(n_cand / TPE_JOINT_CHUNK) 24; it reads
 * n_dims, n_cat, n_quant, n_lattice and chain_len of host_segs and returns
 * TPE_E_ARG for null pointers, n_segs or n_cand < 1, a negative count, counts
 * outside the limits below or a chain_len < 0.  tpe_joint_liar_mseg returns
 * TPE_E_ARG before any launch (no device needed), from the host copies, for
 * everything tpe_joint_liar_seg checks (a continuous group: n_dims in [1,
 * TPE_JOINT_MAX_DIMS]) and per group with n_cat + n_quant > 0: a negative count,
 * n_dims > TPE_JOINT_MSEG_MAX_CONT, n_cat > TPE_JOINT_MSEG_MAX_CAT, n_quant >
 * TPE_JOINT_MAX_QUANT; a psig (continuous or quantised) that is not positive; a
 * U_d outside [2, TPE_JOINT_MAX_CATS] (four of them cannot exceed
 * TPE_JOINT_MAX_CAT_TOTAL), a cat_off that leaves [0, total - U_d], a cat_miss /
 * cat_bonus range that leaves liar_pool; a V_d outside [2, TPE_JOINT_MAX_LATTICE], more than
 * TPE_JOINT_MAX_LATTICE_TOTAL lattice values, an n_lattice that is not sum V_d, a
 * quant_tab_off that is not the running sum of V_d, a quant_edge_off that leaves
 * [0, n_edges - V_d - 1], a quant_edges / above_qmu range that leaves pool_f64
 * (or a null pool_f64), a quant_centre range that leaves liar_pool; a null
 * liar_pool where a group needs it; a row_off, tab_off or sigma_off that is not
 * the running sum.
 * ---------------------------------------------------------------------- */
typedef struct tpe_joint_liar_mseg_desc {
  int32_t n_dims, k_above, n_trials;       /* as tpe_joint_liar_seg_desc ...; n_dims: the continuous labels */
  int32_t chain_len;
  int32_t chain_first;
  int32_t reserved;
  double w_sum, log_w;
  int64_t above_mu;
  int64_t row_off, sigma_off;
  double psig[TPE_JOINT_MAX_DIMS];         /* [d] continuous, [n_dims + d] quantised dimension d */
  double low[TPE_JOINT_MAX_DIMS], high[TPE_JOINT_MAX_DIMS];   /* ... up to here; the continuous bounds */
  int32_t n_cat, n_quant;
  int32_t cat_upper[TPE_JOINT_MSEG_MAX_CAT], cat_off[TPE_JOINT_MSEG_MAX_CAT];   /* as tpe_joint_mseg */
  int32_t quant_v[TPE_JOINT_MAX_QUANT], quant_edge_off[TPE_JOINT_MAX_QUANT];
  int32_t quant_tab_off[TPE_JOINT_MAX_QUANT];   /* start of dimension d in a liar's table and in quant_centre */
  int32_t n_edges, n_lattice;              /* elements of quant_edges; sum_d V_d */
  int64_t above_qmu, quant_edges;          /* element offsets in pool_f64, as tpe_joint_mseg */
  int64_t cat_miss, cat_bonus;             /* element offsets in liar_pool [sum U_d] */
  int64_t quant_centre;                    /* element offset in liar_pool [n_lattice] */
  int64_t tab_off;                         /* doubles: the group's liar tables in scratch [chain_len * n_lattice] */
} tpe_joint_liar_mseg_desc;
typedef struct tpe_joint_liar_mseg_args {
  int32_t n_segs, n_probs, n_cand, reserved;   /* as tpe_joint_liar_seg_args ... */
  const tpe_joint_liar_mseg_desc* segs;        /* device [n_segs], group index order */
  const tpe_joint_liar_mseg_desc* host_segs;   /* host   [n_segs], the same bytes */
  const int32_t* order;
  const int32_t* host_order;
  const int32_t* chain;
  const int32_t* host_chain;
  const double* log_norm;
  const double* host_log_norm;
  const int32_t* host_prob_seg;
  const float* cand;                     /* device, what tpe_joint_mseg_run wrote */
  const int64_t* cand_off;
  const double *l_out, *g_out;
  const float* pool_f32;
  int64_t pool_f32_len;                  /* ... up to here */
  const double* pool_f64;                /* device, tpe_joint_mseg_args.pool_f64 (may be NULL without a quantised group) */
  int64_t pool_f64_len;                  /* elements */
  const double* liar_pool;               /* device f64 (may be NULL with continuous groups only) */
  int64_t liar_pool_len;                 /* elements */
} tpe_joint_liar_mseg_args;

int tpe_joint_liar_mseg_scratch_bytes(const tpe_joint_liar_mseg_desc* host_segs, int32_t n_segs, int32_t n_cand,
                                      uint64_t* bytes);

/* picks: device [n_probs], by problem; pick_z: device f32 [n_probs *
 * TPE_JOINT_MAX_DIMS], problem p's row at p * TPE_JOINT_MAX_DIMS (n_dims + n_cat
 * + n_quant floats written); liar_sigma: device f64 [sum_s chain_len_s (n_dims +
 * n_quant)_s], group s's [chain_len, n_dims + n_quant] rows at sigma_off;
 * enqueued on `stream` */
int tpe_joint_liar_mseg(const tpe_joint_liar_mseg_args* args, tpe_joint_pick* picks, float* pick_z,
                        double* liar_sigma, void* scratch, uint64_t scratch_bytes, void* stream);

/* ------------------------------------------------------------------------
 * Host phase clock of tpe_suggest_tree (tools/native_split.py).  While
 * enabled, a call records the steady-clock microseconds since its entry at
 * each phase below (a tree of several level runs: the last run's phases);
 * phases a call does not reach stay -1.  Process-wide; profiling only.
 * ---------------------------------------------------------------------- */
#define TPE_PHASE_PREFIT   0   /* the up-front fits on the worker threads done   */
#define TPE_PHASE_PACK     1   /* the level packed into the staging buffer       */
#define TPE_PHASE_LAUNCHED 2   /* every kernel of the level issued               */
#define TPE_PHASE_SYNCED   3   /* the stream synchronise returned                */
#define TPE_PHASE_LEVEL    4   /* the level's results assembled                  */
#define TPE_PHASE_RETURN   5   /* tpe_suggest_tree returns                       */
#define TPE_PHASE_RECS     6   /* the level's fits and label records ready (before its pack) */
#define TPE_N_PHASES       7

/* enable (1) / disable (0); *last (if not NULL) gets min(n, TPE_N_PHASES)
 * phase times of the last call (before this one changes the setting) */
int tpe_host_phases(int32_t enable, double* last, int32_t n);

/* ------------------------------------------------------------------------
 * Resident levels.  Of a tpe_suggest_tree call only the Philox key (the seed)
 * and the new ids reach the sample stage afresh; the fits, the packed level
 * and its score tables are a function of the labels' finished trials, the
 * below set, the candidate count and the fit parameters.  The library keeps,
 * per calling thread, a content key of every label's fit (private copies of
 * the scalars and arrays the fit reads: a matching label keeps its fit and its
 * generation) and one record of the last level run (the labels' generations,
 * the run's arguments, every field of its tpe_level_ws, the device, and the
 * process-wide device epoch).  A level run with the same record skips the
 * pack, the upload and the table stage: one small kernel patches key0 / key1 /
 * ctr3 of the device problem rows and selects the lazy categoricals, then the
 * stages run as ever.  A hit with one id across its labels whose stages are the
 * fast sample kernel alone is fused: that kernel takes the three words as launch
 * arguments, the host selects the lazy categoricals while it runs, and the
 * patch kernel is not launched (unless a host selection does not settle within
 * its draw budget: then it runs behind the sample kernel).  Every exported entry that enqueues device work or packs
 * into caller memory advances the epoch, so nothing else can have written
 * under a record that is still alive.  tpe_level_run itself is never resident;
 * levels with device fits, expanded levels, TPE_BATCH_WRITE_CAND levels and
 * candidate-sharded levels are not either.
 *
 * mode 0: off, and drop every record; 1: on (the default); 2: drop only (a
 * caller that rewrites the workspace's blob, tables or staging buffer itself);
 * < 0: query.  stats (if not NULL) gets {hits, misses, fit_reuses, drops}
 * since load.  Returns 1 when the feature is on, else 0.  The environment
 * variable TPE_RESIDENT_LEVEL=0 (read once) keeps it off whatever the mode.
 * ---------------------------------------------------------------------- */
int tpe_level_resident(int32_t mode, int64_t* stats);

/* stats[2] gets {fused hits, fused hits that fell back to the patch kernel}
 * since load (both are also counted among tpe_level_resident's hits).  The
 * environment variable TPE_LAZY_HOST_BUDGET (read per call, part of the
 * record's key) sets the draws the host scans per lazy categorical: 0 makes
 * every fused hit fall back. */
int tpe_level_resident_fused(int64_t* stats);

#ifdef __cplusplus
}
#endif

#endif /* TPE_HIP_H */
