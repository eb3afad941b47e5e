"""ctypes binding of libtpe_hip.so (declared in include/tpe_hip.h).

The library is built in-tree (``__graft_entry__.build()`` or
``python -m hyperopt_amd.build``).  There is no fallback: if the library is
missing or does not load, every suggest call raises ``NativeUnavailable``.
"""
import ctypes
import os

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.environ.get('TPE_HIP_LIB') or os.path.join(HERE, 'libtpe_hip.so')   # override: A/B builds
ABI_VERSION = 24
FIT_DELTA_MAX = 16             # TPE_FIT_DELTA_MAX: new observations read as a delta (no merge)
BEST_PER_TILE = 8         # TPE_BEST_PER_TILE: tile_best slots per candidate tile

FAM_GAUSS, FAM_LOGGAUSS, FAM_QGAUSS, FAM_QLOGGAUSS, FAM_CATEGORICAL = range(5)
F_HAS_LOW, F_HAS_HIGH, F_POOLED, F_CAT_LAZY, F_NO_TABLE, F_PREFIT, F_FGT, F_REMOTE, F_LOGPOLY = \
    1, 2, 4, 8, 16, 32, 64, 128, 256
TAB_NONE, TAB_CELLS, TAB_LATTICE, TAB_LOGPOLY = 0, 1, 2, 3
TAB_PER_BLOCK = 8                  # include/tpe_hip.h TPE_TAB_PER_BLOCK
TAB_ROW_UNITS = 3                  # include/tpe_hip.h TPE_TAB_ROW_UNITS: 16-B units of a cell row
BATCH_NO_EXPAND, BATCH_WRITE_CAND, BATCH_NO_FUSE, BATCH_ORDERED_DRAWS, BATCH_TAB_EXACT, BATCH_NO_TAB_FAST = \
    1, 2, 4, 8, 16, 32
BATCH_NO_FAST2 = 64
PREC_F32, PREC_F64 = 0, 1

# numpy mirrors of the C structs (the host builds arrays of them and copies
# them to device memory in one transfer)
PROBLEM_DTYPE = np.dtype([
    ('family', '<i4'), ('flags', '<i4'), ('n_cand', '<i4'), ('n_upper', '<i4'),
    ('cand_off', '<i8'), ('cand_base', '<i8'), ('n_cand_global', '<i8'),
    ('n_splits', '<i4'), ('tile_off', '<i4'), ('n_tiles', '<i4'), ('samp_off', '<i4'),
    ('samp_len', '<i4'), ('below_off', '<i4'), ('below_len', '<i4'), ('above_off', '<i4'),
    ('above_len', '<i4'), ('wide_off', '<i4'), ('wide_len', '<i4'), ('grid_off', '<i4'),
    ('grid_n', '<i4'), ('sort_slot', '<i4'),
    ('low', '<f8'), ('high', '<f8'), ('q', '<f8'), ('below_base', '<f8'), ('above_base', '<f8'),
    ('prior_mu', '<f4'), ('prior_a', '<f4'), ('prior_c', '<f4'), ('narrow_cmax', '<f4'),
    ('narrow_amin', '<f4'), ('grid_lo', '<f4'), ('grid_inv', '<f4'),
    ('key_lo', '<f4'), ('key_inv', '<f4'), ('pool_first', '<i4'),
    ('key0', '<u4'), ('key1', '<u4'), ('ctr2', '<u4'), ('ctr3', '<u4'),
    ('tab_mode', '<i4'), ('tab_off', '<i4', (2,)), ('tab_n', '<i4', (2,)), ('tab_lo', '<f4', (2,)),
    ('tab_inv', '<f4', (2,)), ('fgt_a', '<f4'), ('lat_lo', '<i8'), ('fgt_off', '<i4'), ('fgt_n', '<i4'),
    ('fgt_lo', '<f8'),
])
assert PROBLEM_DTYPE.itemsize == 256
TAB_JOB_DTYPE = np.dtype([('problem', '<i4'), ('side', '<i4'), ('kind', '<i4'), ('n', '<i4'), ('off', '<i4'),
                          ('block0', '<i4'), ('rows_off', '<i4'), ('rows_n', '<i4'), ('wide_off', '<i4'),
                          ('wide_n', '<i4'), ('lo', '<f4'), ('inv', '<f4')])
assert TAB_JOB_DTYPE.itemsize == 48
TILE_DTYPE = np.dtype([('problem', '<i4'), ('cand_start', '<i4'), ('work_first', '<i4'), ('n_splits', '<i4')])
WORK_DTYPE = np.dtype([('problem', '<i4'), ('split', '<i4'), ('cand_start', '<i4'),
                       ('k_start', '<i4'), ('k_end', '<i4'), ('n_splits', '<i4')])
BEST_DTYPE = np.dtype([('score', '<f8'), ('l', '<f8'), ('g', '<f8'), ('idx', '<i8')])
FIT_JOB_DTYPE = np.dtype([
    ('obs', '<u8'), ('n_obs', '<i8'), ('seg_off', '<i8'), ('below_off', '<i4'), ('n_below', '<i4'),
    ('family', '<i4'), ('flags', '<i4'), ('lf', '<i4'), ('problem_first', '<i4'), ('n_problems', '<i4'),
    ('above_off', '<i4'), ('wide_off', '<i4'), ('grid_off', '<i4'), ('grid_n', '<i4'), ('reserved', '<i4'),
    ('prior_mu', '<f8'), ('prior_sigma', '<f8'), ('prior_weight', '<f8'), ('low', '<f8'), ('high', '<f8'),
    ('ord_key_in', '<u8'), ('ord_idx_in', '<u8'), ('n_ord_in', '<i8'), ('ord_key_out', '<u8'), ('ord_idx_out', '<u8'),
])
assert FIT_JOB_DTYPE.itemsize == 152
RESULT_DTYPE = np.dtype([('score', '<f8'), ('l', '<f8'), ('g', '<f8'), ('value', '<f8'),
                         ('idx', '<i8'), ('global_idx', '<i8')])
assert RESULT_DTYPE.itemsize == 48
# candidate report (include/tpe_hip.h "Candidate report")
REPORT_CHUNK = 4096            # TPE_REPORT_CHUNK: candidates per pass-1 workgroup
REPORT_MAX_K = 64              # TPE_REPORT_MAX_K
TOP_ENTRY_DTYPE = np.dtype([('value', '<f8'), ('l', '<f8'), ('g', '<f8'), ('global_idx', '<i8')])
assert TOP_ENTRY_DTYPE.itemsize == 32
SCORE_STATS_DTYPE = np.dtype([('n_finite', '<i8'), ('n_nan', '<i8'), ('n_posinf', '<i8'), ('n_neginf', '<i8'),
                              ('mean', '<f8'), ('m2', '<f8'), ('min', '<f8'), ('max', '<f8')])
assert SCORE_STATS_DTYPE.itemsize == 64
# joint TPE stage (include/tpe_hip.h "Joint (multivariate) TPE stage")
JOINT_MAX_DIMS = 16            # TPE_JOINT_MAX_DIMS
JOINT_CHUNK = 1024             # TPE_JOINT_CHUNK: candidates per workgroup
JOINT_STREAM = 0xFFFFFFFF      # TPE_JOINT_STREAM: the Philox counter word no label index equals
JOINT_INJECT = 1               # TPE_JOINT_INJECT
JOINT_RECORD_DTYPE = np.dtype([('global_idx', '<i8'), ('l', '<f8'), ('g', '<f8'), ('z', '<f8', (JOINT_MAX_DIMS,))])
assert JOINT_RECORD_DTYPE.itemsize == 152
JOINT_MAX_CATS = 256           # TPE_JOINT_MAX_CATS: categories of one joined discrete label
JOINT_MAX_CAT_TOTAL = 1024     # TPE_JOINT_MAX_CAT_TOTAL: categories of a joint group
JOINT_MAX_QUANT = 4            # TPE_JOINT_MAX_QUANT: quantised labels of a joint group
JOINT_MAX_LATTICE = 256        # TPE_JOINT_MAX_LATTICE: lattice values of one joined quantised label
JOINT_MAX_LATTICE_TOTAL = 512  # TPE_JOINT_MAX_LATTICE_TOTAL: lattice values of a joint group
JOINT_QFLOOR = -4096.0         # TPE_JOINT_QFLOOR: the smallest stored log2 P_kd(i)
JOINT_QUANT_MAX_CONT = 8       # continuous / discrete labels beside a quantised one
JOINT_QUANT_MAX_DISC = 4
JOINT_WIDE_MAX_DIMS = 64       # TPE_JOINT_WIDE_MAX_DIMS: labels of a wide joint group
JOINT_WIDE_MAX_CAT = 8         # TPE_JOINT_WIDE_MAX_CAT: discrete labels among them (tpe_joint_wide_mixed_run)
JOINT_WIDE_RECORD_DTYPE = np.dtype([('global_idx', '<i8'), ('l', '<f8'), ('g', '<f8'),
                                    ('z', '<f8', (JOINT_WIDE_MAX_DIMS,))])
assert JOINT_WIDE_RECORD_DTYPE.itemsize == 536
# joint candidate report (include/tpe_hip.h "Joint candidate report")
JOINT_REPORT_CHUNK = 4096      # TPE_JOINT_REPORT_CHUNK: candidates per pass-1 workgroup
JOINT_TOP_ENTRY_DTYPE = np.dtype([('idx', '<i8'), ('l', '<f8'), ('g', '<f8'), ('reserved', '<i8')])
assert JOINT_TOP_ENTRY_DTYPE.itemsize == 32


class Batch(ctypes.Structure):
    _fields_ = [
        ('problems', ctypes.c_void_p), ('n_problems', ctypes.c_int32),
        ('precision', ctypes.c_int32), ('sample', ctypes.c_int32), ('sort_end_bit', ctypes.c_int32),
        ('key_bits', ctypes.c_int32), ('flags', ctypes.c_int32),
        ('comp32', ctypes.c_void_p), ('comp64', ctypes.c_void_p), ('samp', ctypes.c_void_p),
        ('grid', ctypes.c_void_p),
        ('cand', ctypes.c_void_p), ('coord', ctypes.c_void_p),
        ('keys', ctypes.c_void_p), ('vals', ctypes.c_void_p),
        ('keys_sorted', ctypes.c_void_p), ('vals_sorted', ctypes.c_void_p),
        ('sort_tmp', ctypes.c_void_p), ('sort_tmp_bytes', ctypes.c_uint64),
        ('total_cand', ctypes.c_int64),
        ('tiles', ctypes.c_void_p), ('n_tiles', ctypes.c_int32), ('n_fin_tiles', ctypes.c_int32),
        ('sort_count', ctypes.c_int64), ('fin_tiles', ctypes.c_void_p),
        ('work', ctypes.c_void_p),
        ('n_work_cont', ctypes.c_int32), ('n_work_qgauss', ctypes.c_int32),
        ('n_work_qlog', ctypes.c_int32), ('fgt_max_boxes', ctypes.c_int32),
        ('part', ctypes.c_void_p), ('l_out', ctypes.c_void_p), ('g_out', ctypes.c_void_p),
        ('tile_best', ctypes.c_void_p), ('result', ctypes.c_void_p),
        ('ce_count', ctypes.c_void_p),
        ('fit', ctypes.c_void_p), ('n_fit', ctypes.c_int32), ('fgt_max_cells', ctypes.c_int32),
        ('below_idx', ctypes.c_void_p), ('fit_seg', ctypes.c_void_p), ('fit_total', ctypes.c_int64),
        ('fit_keys', ctypes.c_void_p), ('fit_keys_sorted', ctypes.c_void_p),
        ('fit_vals', ctypes.c_void_p), ('fit_vals_sorted', ctypes.c_void_p),
        ('fit_max_new', ctypes.c_int64), ('fit_max_obs', ctypes.c_int64), ('fit_max_merge', ctypes.c_int64),
        ('fit_n_delta', ctypes.c_int64),
        ('draw_pref', ctypes.c_void_p), ('draw_blocks', ctypes.c_int64), ('n_sorted', ctypes.c_int32),
        ('tab_fast', ctypes.c_int32), ('pool_best', ctypes.c_void_p),
        ('tab_jobs', ctypes.c_void_p), ('n_tab_jobs', ctypes.c_int32), ('tab_blocks', ctypes.c_int32),
        ('tab', ctypes.c_void_p), ('tab_units', ctypes.c_int64),
        ('samp_tiles', ctypes.c_void_p), ('n_samp_tiles', ctypes.c_int32), ('n_samp_eager', ctypes.c_int32),
        ('tab_tiles', ctypes.c_void_p), ('n_tab_tiles', ctypes.c_int32), ('early_select', ctypes.c_int32),
        ('run_best', ctypes.c_void_p), ('n_late', ctypes.c_int32), ('tiles_per_problem', ctypes.c_int32),
    ]


class JointArgs(ctypes.Structure):
    """tpe_joint_args: one tpe_joint_run."""
    _fields_ = [
        ('n_dims', ctypes.c_int32), ('n_cand', ctypes.c_int32), ('n_ids', ctypes.c_int32), ('flags', ctypes.c_int32),
        ('k_below', ctypes.c_int32), ('k_above', ctypes.c_int32), ('stream_word', ctypes.c_uint32),
        ('reserved', ctypes.c_int32), ('seed', ctypes.c_uint64),
        ('below_mu', ctypes.c_void_p), ('below_a', ctypes.c_void_p), ('below_c', ctypes.c_void_p),
        ('above_mu', ctypes.c_void_p), ('above_a', ctypes.c_void_p), ('above_c', ctypes.c_void_p),
        ('below_base', ctypes.c_double), ('above_base', ctypes.c_double),
        ('samp_cum', ctypes.c_void_p), ('samp', ctypes.c_void_p), ('ids', ctypes.c_void_p),
        ('inject', ctypes.c_void_p),
        ('low', ctypes.c_double * JOINT_MAX_DIMS), ('high', ctypes.c_double * JOINT_MAX_DIMS),
    ]


class JointWideArgs(ctypes.Structure):
    """tpe_joint_wide_args: one tpe_joint_wide_run (tpe_joint_args with 64 bounds)."""
    _fields_ = JointArgs._fields_[:-2] + [
        ('low', ctypes.c_double * JOINT_WIDE_MAX_DIMS), ('high', ctypes.c_double * JOINT_WIDE_MAX_DIMS),
    ]


class JointMixedArgs(ctypes.Structure):
    """tpe_joint_mixed_args: one tpe_joint_mixed_run (n_dims continuous, n_cat discrete labels)."""
    _fields_ = [
        ('n_dims', ctypes.c_int32), ('n_cand', ctypes.c_int32), ('n_ids', ctypes.c_int32), ('flags', ctypes.c_int32),
        ('k_below', ctypes.c_int32), ('k_above', ctypes.c_int32), ('stream_word', ctypes.c_uint32),
        ('n_cat', ctypes.c_int32), ('seed', ctypes.c_uint64),
        ('below_mu', ctypes.c_void_p), ('below_a', ctypes.c_void_p), ('below_c', ctypes.c_void_p),
        ('above_mu', ctypes.c_void_p), ('above_a', ctypes.c_void_p), ('above_c', ctypes.c_void_p),
        ('below_base', ctypes.c_double), ('above_base', ctypes.c_double),
        ('samp_cum', ctypes.c_void_p), ('samp', ctypes.c_void_p), ('ids', ctypes.c_void_p),
        ('inject', ctypes.c_void_p),
        ('low', ctypes.c_double * JOINT_MAX_DIMS), ('high', ctypes.c_double * JOINT_MAX_DIMS),
        ('cat_upper', ctypes.c_int32 * JOINT_MAX_DIMS), ('cat_off', ctypes.c_int32 * JOINT_MAX_DIMS),
        ('below_cat', ctypes.c_void_p), ('above_cat', ctypes.c_void_p),
        ('below_miss', ctypes.c_void_p), ('below_bonus', ctypes.c_void_p),
        ('above_miss', ctypes.c_void_p), ('above_bonus', ctypes.c_void_p),
        ('below_h', ctypes.c_void_p), ('cat_cum', ctypes.c_void_p),
    ]


class JointWideMixedArgs(ctypes.Structure):
    """tpe_joint_wide_mixed_args: one tpe_joint_wide_mixed_run (tpe_joint_wide_args' fields, then up to
    JOINT_WIDE_MAX_CAT discrete labels and the mixed stage's tables)."""
    _fields_ = JointWideArgs._fields_ + [
        ('n_cat', ctypes.c_int32),
        ('cat_upper', ctypes.c_int32 * JOINT_WIDE_MAX_CAT), ('cat_off', ctypes.c_int32 * JOINT_WIDE_MAX_CAT),
    ] + JointMixedArgs._fields_[-8:]


class JointQuantArgs(ctypes.Structure):
    """tpe_joint_quant_args: one tpe_joint_quant_run (tpe_joint_mixed_args' fields, then the quantised labels')."""
    _fields_ = JointMixedArgs._fields_ + [
        ('n_quant', ctypes.c_int32), ('n_edges', ctypes.c_int32),
        ('quant_v', ctypes.c_int32 * JOINT_MAX_QUANT), ('quant_edge_off', ctypes.c_int32 * JOINT_MAX_QUANT),
        ('quant_edges', ctypes.c_void_p),
        ('below_qmu', ctypes.c_void_p), ('below_qsigma', ctypes.c_void_p),
        ('above_qmu', ctypes.c_void_p), ('above_qsigma', ctypes.c_void_p),
        ('quant_samp', ctypes.c_void_p), ('quant_table', ctypes.c_void_p), ('quant_table_bytes', ctypes.c_uint64),
    ]


class JointWideQuantArgs(ctypes.Structure):
    """tpe_joint_wide_quant_args: one tpe_joint_wide_quant_run (tpe_joint_wide_mixed_args' fields, then the
    quantised labels' of tpe_joint_quant_args)."""
    _fields_ = JointWideMixedArgs._fields_ + JointQuantArgs._fields_[len(JointMixedArgs._fields_):]


class JointSeg(ctypes.Structure):
    """tpe_joint_seg: the device descriptor of one group of a tpe_joint_seg_run."""
    _fields_ = [
        ('n_dims', ctypes.c_int32), ('k_below', ctypes.c_int32), ('k_above', ctypes.c_int32),
        ('stream_word', ctypes.c_uint32),
        ('below_base', ctypes.c_double), ('above_base', ctypes.c_double),
        ('below_mu', ctypes.c_int64), ('below_a', ctypes.c_int64), ('below_c', ctypes.c_int64),
        ('above_mu', ctypes.c_int64), ('above_a', ctypes.c_int64), ('above_c', ctypes.c_int64),
        ('samp', ctypes.c_int64), ('inject', ctypes.c_int64), ('samp_cum', ctypes.c_int64),
        ('lo', ctypes.c_float * JOINT_MAX_DIMS), ('hi', ctypes.c_float * JOINT_MAX_DIMS),
    ]


# numpy mirror of tpe_joint_seg (an array of them is uploaded in one transfer)
JOINT_SEG_DTYPE = np.dtype([
    ('n_dims', '<i4'), ('k_below', '<i4'), ('k_above', '<i4'), ('stream_word', '<u4'),
    ('below_base', '<f8'), ('above_base', '<f8'),
    ('below_mu', '<i8'), ('below_a', '<i8'), ('below_c', '<i8'),
    ('above_mu', '<i8'), ('above_a', '<i8'), ('above_c', '<i8'),
    ('samp', '<i8'), ('inject', '<i8'), ('samp_cum', '<i8'),
    ('lo', '<f4', (JOINT_MAX_DIMS,)), ('hi', '<f4', (JOINT_MAX_DIMS,))])
assert JOINT_SEG_DTYPE.itemsize == ctypes.sizeof(JointSeg) == 232


class JointSegArgs(ctypes.Structure):
    """tpe_joint_seg_args: one tpe_joint_seg_run."""
    _fields_ = [
        ('n_segs', ctypes.c_int32), ('n_probs', ctypes.c_int32), ('n_cand', ctypes.c_int32), ('flags', ctypes.c_int32),
        ('seed', ctypes.c_uint64),
        ('segs', ctypes.c_void_p), ('host_segs', ctypes.c_void_p),
        ('pool_f32', ctypes.c_void_p), ('pool_f64', ctypes.c_void_p),
        ('pool_f32_len', ctypes.c_int64), ('pool_f64_len', ctypes.c_int64),
        ('prob_seg', ctypes.c_void_p), ('host_prob_seg', ctypes.c_void_p),
        ('prob_id', ctypes.c_void_p), ('cand_off', ctypes.c_void_p),
    ]


class JointWideSeg(ctypes.Structure):
    """tpe_joint_wide_seg: the device descriptor of one group of a tpe_joint_wide_seg_run (tpe_joint_seg with
    JOINT_WIDE_MAX_DIMS bounds)."""
    _fields_ = JointSeg._fields_[:-2] + [
        ('lo', ctypes.c_float * JOINT_WIDE_MAX_DIMS), ('hi', ctypes.c_float * JOINT_WIDE_MAX_DIMS)]


# numpy mirror of tpe_joint_wide_seg
JOINT_WIDE_SEG_DTYPE = np.dtype(JOINT_SEG_DTYPE.descr[:-2] + [
    ('lo', '<f4', (JOINT_WIDE_MAX_DIMS,)), ('hi', '<f4', (JOINT_WIDE_MAX_DIMS,))])
assert JOINT_WIDE_SEG_DTYPE.itemsize == ctypes.sizeof(JointWideSeg) == 616


class JointWideSegArgs(ctypes.Structure):
    """tpe_joint_wide_seg_args: one tpe_joint_wide_seg_run (tpe_joint_seg_args' fields)."""
    _fields_ = list(JointSegArgs._fields_)


JOINT_MSEG_MAX_CONT = 8        # TPE_JOINT_MSEG_MAX_CONT: continuous coordinates beside a discrete / quantised one
JOINT_MSEG_MAX_CAT = 4         # TPE_JOINT_MSEG_MAX_CAT: discrete coordinates of a segment


class JointMSeg(ctypes.Structure):
    """tpe_joint_mseg: the device descriptor of one group of a tpe_joint_mseg_run (tpe_joint_seg's fields first)."""
    _fields_ = JointSeg._fields_ + [
        ('n_cat', ctypes.c_int32), ('n_quant', ctypes.c_int32),
        ('cat_upper', ctypes.c_int32 * JOINT_MSEG_MAX_CAT), ('cat_off', ctypes.c_int32 * JOINT_MSEG_MAX_CAT),
        ('quant_v', ctypes.c_int32 * JOINT_MAX_QUANT), ('quant_edge_off', ctypes.c_int32 * JOINT_MAX_QUANT),
        ('qlo', ctypes.c_float * JOINT_MAX_QUANT), ('qhi', ctypes.c_float * JOINT_MAX_QUANT),
        ('n_edges', ctypes.c_int32), ('reserved', ctypes.c_int32),
        ('below_cat', ctypes.c_int64), ('above_cat', ctypes.c_int64),
        ('below_miss', ctypes.c_int64), ('below_bonus', ctypes.c_int64),
        ('above_miss', ctypes.c_int64), ('above_bonus', ctypes.c_int64),
        ('quant_samp', ctypes.c_int64), ('below_h', ctypes.c_int64), ('cat_cum', ctypes.c_int64),
        ('quant_edges', ctypes.c_int64),
        ('below_qmu', ctypes.c_int64), ('below_qsigma', ctypes.c_int64),
        ('above_qmu', ctypes.c_int64), ('above_qsigma', ctypes.c_int64),
        ('table', ctypes.c_int64),
    ]


# numpy mirror of tpe_joint_mseg
JOINT_MSEG_DTYPE = np.dtype(JOINT_SEG_DTYPE.descr + [
    ('n_cat', '<i4'), ('n_quant', '<i4'),
    ('cat_upper', '<i4', (JOINT_MSEG_MAX_CAT,)), ('cat_off', '<i4', (JOINT_MSEG_MAX_CAT,)),
    ('quant_v', '<i4', (JOINT_MAX_QUANT,)), ('quant_edge_off', '<i4', (JOINT_MAX_QUANT,)),
    ('qlo', '<f4', (JOINT_MAX_QUANT,)), ('qhi', '<f4', (JOINT_MAX_QUANT,)),
    ('n_edges', '<i4'), ('reserved', '<i4'),
    ('below_cat', '<i8'), ('above_cat', '<i8'), ('below_miss', '<i8'), ('below_bonus', '<i8'),
    ('above_miss', '<i8'), ('above_bonus', '<i8'), ('quant_samp', '<i8'), ('below_h', '<i8'), ('cat_cum', '<i8'),
    ('quant_edges', '<i8'), ('below_qmu', '<i8'), ('below_qsigma', '<i8'), ('above_qmu', '<i8'),
    ('above_qsigma', '<i8'), ('table', '<i8')])
assert JOINT_MSEG_DTYPE.itemsize == ctypes.sizeof(JointMSeg) == 464


class JointMSegArgs(ctypes.Structure):
    """tpe_joint_mseg_args: one tpe_joint_mseg_run (tpe_joint_seg_args' fields, then the table workspace)."""
    _fields_ = JointSegArgs._fields_ + [('quant_table', ctypes.c_void_p), ('quant_table_bytes', ctypes.c_uint64)]


# tpe_joint_run_shard (include/tpe_hip.h "Sharded joint stage"): the stage whose args and records a call takes
JOINT_STAGE_RUN, JOINT_STAGE_WIDE, JOINT_STAGE_MIXED, JOINT_STAGE_QUANT, JOINT_STAGE_SEG, JOINT_STAGE_MSEG = range(6)
# the stage of each stage entry point, by its name
JOINT_STAGES = {'tpe_joint_run': JOINT_STAGE_RUN, 'tpe_joint_wide_run': JOINT_STAGE_WIDE,
                'tpe_joint_mixed_run': JOINT_STAGE_MIXED, 'tpe_joint_quant_run': JOINT_STAGE_QUANT,
                'tpe_joint_seg_run': JOINT_STAGE_SEG, 'tpe_joint_mseg_run': JOINT_STAGE_MSEG}


class JointShard(ctypes.Structure):
    """tpe_joint_shard: the candidates [cand_base, cand_base + args.n_cand) of n_cand_global."""
    _fields_ = [('cand_base', ctypes.c_int64), ('n_cand_global', ctypes.c_int64)]


class JointReportArgs(ctypes.Structure):
    """tpe_joint_report_args: one tpe_joint_report."""
    _fields_ = [
        ('n_probs', ctypes.c_int32), ('n_cand', ctypes.c_int32), ('width', ctypes.c_int32),
        ('z_stride', ctypes.c_int32),
        ('cand', ctypes.c_void_p), ('l_out', ctypes.c_void_p), ('g_out', ctypes.c_void_p),
        ('cand_off', ctypes.c_void_p), ('widths', ctypes.c_void_p), ('host_widths', ctypes.c_void_p),
    ]


JOINT_LIAR_TILE = 32   # TPE_JOINT_LIAR_TILE
JOINT_PICK_DTYPE = np.dtype([('idx', '<i8'), ('l', '<f8'), ('g', '<f8')])
assert JOINT_PICK_DTYPE.itemsize == 24


class JointLiarArgs(ctypes.Structure):
    """tpe_joint_liar_args: one tpe_joint_liar."""
    _fields_ = [
        ('n_dims', ctypes.c_int32), ('n_cand', ctypes.c_int32), ('n_ids', ctypes.c_int32), ('n_given', ctypes.c_int32),
        ('k_above', ctypes.c_int32), ('n_trials', ctypes.c_int32),
        ('w_sum', ctypes.c_double),
        ('cand', ctypes.c_void_p), ('l_out', ctypes.c_void_p), ('g_out', ctypes.c_void_p),
        ('above_mu', ctypes.c_void_p), ('given', ctypes.c_void_p),
        ('psig', ctypes.c_double * 64), ('low', ctypes.c_double * 64), ('high', ctypes.c_double * 64),
    ]


class JointLiarMixedArgs(ctypes.Structure):
    """tpe_joint_liar_mixed_args: one tpe_joint_liar_mixed (tpe_joint_liar_args' fields, then the discrete and
    quantised labels')."""
    _fields_ = JointLiarArgs._fields_ + [
        ('n_cat', ctypes.c_int32), ('n_quant', ctypes.c_int32),
        ('cat_upper', ctypes.c_int32 * JOINT_MAX_DIMS), ('cat_off', ctypes.c_int32 * JOINT_MAX_DIMS),
        ('cat_miss', ctypes.c_void_p), ('cat_bonus', ctypes.c_void_p),
        ('quant_v', ctypes.c_int32 * JOINT_MAX_QUANT), ('quant_edge_off', ctypes.c_int32 * JOINT_MAX_QUANT),
        ('n_edges', ctypes.c_int32), ('reserved', ctypes.c_int32),
        ('quant_edges', ctypes.c_void_p), ('quant_centre', ctypes.c_void_p), ('above_qmu', ctypes.c_void_p),
    ]


class JointLiarSeg(ctypes.Structure):
    """tpe_joint_liar_seg_desc: the device descriptor of one group of a tpe_joint_liar_seg."""
    _fields_ = [
        ('n_dims', ctypes.c_int32), ('k_above', ctypes.c_int32), ('n_trials', ctypes.c_int32),
        ('chain_len', ctypes.c_int32), ('chain_first', ctypes.c_int32), ('reserved', ctypes.c_int32),
        ('w_sum', ctypes.c_double), ('log_w', ctypes.c_double),
        ('above_mu', ctypes.c_int64), ('row_off', ctypes.c_int64), ('sigma_off', ctypes.c_int64),
        ('psig', ctypes.c_double * JOINT_MAX_DIMS), ('low', ctypes.c_double * JOINT_MAX_DIMS),
        ('high', ctypes.c_double * JOINT_MAX_DIMS),
    ]


# numpy mirror of tpe_joint_liar_seg_desc (an array of them is uploaded in one transfer)
JOINT_LIAR_SEG_DTYPE = np.dtype([
    ('n_dims', '<i4'), ('k_above', '<i4'), ('n_trials', '<i4'), ('chain_len', '<i4'), ('chain_first', '<i4'),
    ('reserved', '<i4'), ('w_sum', '<f8'), ('log_w', '<f8'), ('above_mu', '<i8'), ('row_off', '<i8'),
    ('sigma_off', '<i8'), ('psig', '<f8', (JOINT_MAX_DIMS,)), ('low', '<f8', (JOINT_MAX_DIMS,)),
    ('high', '<f8', (JOINT_MAX_DIMS,))])
assert JOINT_LIAR_SEG_DTYPE.itemsize == ctypes.sizeof(JointLiarSeg) == 448


class JointLiarSegArgs(ctypes.Structure):
    """tpe_joint_liar_seg_args: one tpe_joint_liar_seg."""
    _fields_ = [
        ('n_segs', ctypes.c_int32), ('n_probs', ctypes.c_int32), ('n_cand', ctypes.c_int32),
        ('reserved', ctypes.c_int32),
        ('segs', ctypes.c_void_p), ('host_segs', ctypes.c_void_p),
        ('order', ctypes.c_void_p), ('host_order', ctypes.c_void_p),
        ('chain', ctypes.c_void_p), ('host_chain', ctypes.c_void_p),
        ('log_norm', ctypes.c_void_p), ('host_log_norm', ctypes.c_void_p),
        ('host_prob_seg', ctypes.c_void_p),
        ('cand', ctypes.c_void_p), ('cand_off', ctypes.c_void_p), ('l_out', ctypes.c_void_p),
        ('g_out', ctypes.c_void_p), ('pool_f32', ctypes.c_void_p), ('pool_f32_len', ctypes.c_int64),
    ]


class JointLiarMSeg(ctypes.Structure):
    """tpe_joint_liar_mseg_desc: the device descriptor of one group of a tpe_joint_liar_mseg (JointLiarSeg's fields
    first)."""
    _fields_ = JointLiarSeg._fields_ + [
        ('n_cat', ctypes.c_int32), ('n_quant', ctypes.c_int32),
        ('cat_upper', ctypes.c_int32 * JOINT_MSEG_MAX_CAT), ('cat_off', ctypes.c_int32 * JOINT_MSEG_MAX_CAT),
        ('quant_v', ctypes.c_int32 * JOINT_MAX_QUANT), ('quant_edge_off', ctypes.c_int32 * JOINT_MAX_QUANT),
        ('quant_tab_off', ctypes.c_int32 * JOINT_MAX_QUANT),
        ('n_edges', ctypes.c_int32), ('n_lattice', ctypes.c_int32),
        ('above_qmu', ctypes.c_int64), ('quant_edges', ctypes.c_int64),
        ('cat_miss', ctypes.c_int64), ('cat_bonus', ctypes.c_int64), ('quant_centre', ctypes.c_int64),
        ('tab_off', ctypes.c_int64),
    ]


# numpy mirror of tpe_joint_liar_mseg_desc
JOINT_LIAR_MSEG_DTYPE = np.dtype(JOINT_LIAR_SEG_DTYPE.descr + [
    ('n_cat', '<i4'), ('n_quant', '<i4'),
    ('cat_upper', '<i4', (JOINT_MSEG_MAX_CAT,)), ('cat_off', '<i4', (JOINT_MSEG_MAX_CAT,)),
    ('quant_v', '<i4', (JOINT_MAX_QUANT,)), ('quant_edge_off', '<i4', (JOINT_MAX_QUANT,)),
    ('quant_tab_off', '<i4', (JOINT_MAX_QUANT,)), ('n_edges', '<i4'), ('n_lattice', '<i4'),
    ('above_qmu', '<i8'), ('quant_edges', '<i8'), ('cat_miss', '<i8'), ('cat_bonus', '<i8'), ('quant_centre', '<i8'),
    ('tab_off', '<i8')])
assert JOINT_LIAR_MSEG_DTYPE.itemsize == ctypes.sizeof(JointLiarMSeg) == 592


class JointLiarMSegArgs(ctypes.Structure):
    """tpe_joint_liar_mseg_args: one tpe_joint_liar_mseg (tpe_joint_liar_seg_args' fields, then the f64 pools)."""
    _fields_ = JointLiarSegArgs._fields_ + [
        ('pool_f64', ctypes.c_void_p), ('pool_f64_len', ctypes.c_int64),
        ('liar_pool', ctypes.c_void_p), ('liar_pool_len', ctypes.c_int64),
    ]


class LabelIn(ctypes.Structure):
    _fields_ = [
        ('family', ctypes.c_int32), ('flags', ctypes.c_int32), ('upper', ctypes.c_int32),
        ('label_ix', ctypes.c_int32),
        ('low', ctypes.c_double), ('high', ctypes.c_double), ('q', ctypes.c_double),
        ('below_w', ctypes.c_void_p), ('below_mu', ctypes.c_void_p), ('below_sigma', ctypes.c_void_p),
        ('below_k', ctypes.c_int64),
        ('above_w', ctypes.c_void_p), ('above_mu', ctypes.c_void_p), ('above_sigma', ctypes.c_void_p),
        ('above_k', ctypes.c_int64),
        ('ids', ctypes.c_void_p), ('n_ids', ctypes.c_int64),
        ('dev_obs', ctypes.c_void_p), ('n_obs', ctypes.c_int64),
        ('below_idx', ctypes.c_void_p), ('n_below', ctypes.c_int32), ('lf', ctypes.c_int32),
        ('prior_mu', ctypes.c_double), ('prior_sigma', ctypes.c_double), ('prior_weight', ctypes.c_double),
        ('ord_key_in', ctypes.c_void_p), ('ord_idx_in', ctypes.c_void_p), ('n_ord_in', ctypes.c_int64),
        ('ord_key_out', ctypes.c_void_p), ('ord_idx_out', ctypes.c_void_p),
    ]


def _dtype_of(struct):
    """numpy mirror of a ctypes Structure (pointers as uint64): lets a whole
    array of structs be filled with one tuple assignment per element."""
    conv = {ctypes.c_int32: '<i4', ctypes.c_int64: '<i8', ctypes.c_double: '<f8', ctypes.c_void_p: '<u8',
            ctypes.c_uint64: '<u8'}
    names, formats, offsets = [], [], []
    for name, ct in struct._fields_:
        names.append(name)
        formats.append(conv[ct])
        offsets.append(getattr(struct, name).offset)
    return np.dtype(dict(names=names, formats=formats, offsets=offsets, itemsize=ctypes.sizeof(struct)))


LABEL_DTYPE = _dtype_of(LabelIn)


class PackInfo(ctypes.Structure):
    _fields_ = [
        ('off_problems', ctypes.c_int64), ('off_tiles', ctypes.c_int64), ('off_work', ctypes.c_int64),
        ('off_comp32', ctypes.c_int64), ('off_comp64', ctypes.c_int64), ('off_samp', ctypes.c_int64),
        ('off_grid', ctypes.c_int64), ('n_problems', ctypes.c_int64), ('n_tiles', ctypes.c_int64),
        ('n_work_cont', ctypes.c_int32), ('n_work_qgauss', ctypes.c_int32), ('n_work_qlog', ctypes.c_int32),
        ('any_pruned', ctypes.c_int32), ('part_total', ctypes.c_int64), ('blob_bytes', ctypes.c_int64),
        ('key_bits', ctypes.c_int32), ('sort_end_bit', ctypes.c_int32),
        ('off_fit', ctypes.c_int64), ('off_below_idx', ctypes.c_int64), ('off_fit_seg', ctypes.c_int64),
        ('n_fit', ctypes.c_int32), ('fgt_max_boxes', ctypes.c_int32), ('fit_total', ctypes.c_int64),
        ('sort_count', ctypes.c_int64),
        ('off_fin_tiles', ctypes.c_int64), ('n_fin_tiles', ctypes.c_int64), ('fit_max_new', ctypes.c_int64),
        ('fit_max_obs', ctypes.c_int64), ('fit_max_merge', ctypes.c_int64), ('fit_n_delta', ctypes.c_int64),
        ('n_sorted', ctypes.c_int64), ('draw_blocks', ctypes.c_int64), ('n_pooled', ctypes.c_int64),
        ('off_tab_jobs', ctypes.c_int64), ('n_tab_jobs', ctypes.c_int64), ('tab_blocks', ctypes.c_int64),
        ('tab_units', ctypes.c_int64),
        ('off_samp_tiles', ctypes.c_int64), ('n_samp_tiles', ctypes.c_int64), ('n_samp_eager', ctypes.c_int64),
        ('off_tab_tiles', ctypes.c_int64), ('n_tab_tiles', ctypes.c_int64),
        ('off_expand', ctypes.c_int64), ('n_expand', ctypes.c_int64),
        ('fgt_max_cells', ctypes.c_int64),
        ('up_off', ctypes.c_int64 * 4), ('up_len', ctypes.c_int64 * 4), ('n_up', ctypes.c_int32),
        ('pad_', ctypes.c_int32), ('off_patch', ctypes.c_int64),
    ]


class LevelWS(ctypes.Structure):
    """tpe_level_ws: caller-owned buffers of tpe_level_run."""
    _fields_ = [
        ('pinned', ctypes.c_void_p), ('pinned_bytes', ctypes.c_int64), ('pinned_dev', ctypes.c_void_p),
        ('blob', ctypes.c_void_p), ('blob_bytes', ctypes.c_int64),
        ('cand', ctypes.c_void_p), ('coord', ctypes.c_void_p),
        ('keys', ctypes.c_void_p), ('vals', ctypes.c_void_p), ('keys_sorted', ctypes.c_void_p),
        ('vals_sorted', ctypes.c_void_p), ('cand_cap', ctypes.c_int64),
        ('sort_tmp', ctypes.c_void_p), ('sort_tmp_bytes', ctypes.c_int64),
        ('part', ctypes.c_void_p), ('part_cap', ctypes.c_int64),
        ('tile_best', ctypes.c_void_p), ('best_cap', ctypes.c_int64),
        ('result', ctypes.c_void_p), ('result_cap', ctypes.c_int64),
        ('fit_keys', ctypes.c_void_p), ('fit_keys_sorted', ctypes.c_void_p),
        ('fit_vals', ctypes.c_void_p), ('fit_vals_sorted', ctypes.c_void_p), ('fit_cap', ctypes.c_int64),
        ('draw_pref', ctypes.c_void_p), ('draw_pref_cap', ctypes.c_int64),
        ('pool_best', ctypes.c_void_p), ('pool_best_cap', ctypes.c_int64),
        ('tab', ctypes.c_void_p), ('tab_cap', ctypes.c_int64),
    ]


class LevelNeed(ctypes.Structure):
    """tpe_level_need: sizes one level needs."""
    _fields_ = [(k, ctypes.c_int64) for k in ('pinned_bytes', 'blob_bytes', 'cand', 'sort_tmp_bytes', 'part',
                                              'best', 'result', 'fit',
                                              'draw_pref', 'pool_best', 'tab')]


E_HIP = -2
E_SPACE = -4
E_FALLBACK = -5          # tpe_suggest_tree: the space / history needs the general (host) path
TREE_MAX_PARENTS = 4
TREE_NO_SPECULATE = 1 << 8


class TreeLabel(ctypes.Structure):
    """tpe_tree_label: one hyperparameter of a tree space (tpe_suggest_tree)."""
    _fields_ = [
        ('family', ctypes.c_int32), ('flags', ctypes.c_int32), ('upper', ctypes.c_int32),
        ('label_ix', ctypes.c_int32),
        ('low', ctypes.c_double), ('high', ctypes.c_double), ('prior_mu', ctypes.c_double),
        ('prior_sigma', ctypes.c_double),
        ('p_prior', ctypes.c_void_p), ('tids', ctypes.c_void_p), ('values', ctypes.c_void_p),
        ('order', ctypes.c_void_p), ('n_obs', ctypes.c_int64),
        ('depth', ctypes.c_int32), ('n_parents', ctypes.c_int32),
        ('parent', ctypes.c_int32 * TREE_MAX_PARENTS), ('parent_cat', ctypes.c_int32 * TREE_MAX_PARENTS),
        ('q', ctypes.c_double),
        ('host_w', ctypes.c_void_p * 2), ('host_mu', ctypes.c_void_p * 2), ('host_sigma', ctypes.c_void_p * 2),
        ('host_k', ctypes.c_int64 * 2),
        ('dev_obs', ctypes.c_void_p), ('ord_key_in', ctypes.c_void_p), ('ord_idx_in', ctypes.c_void_p),
        ('n_ord_in', ctypes.c_int64), ('ord_key_out', ctypes.c_void_p), ('ord_idx_out', ctypes.c_void_p),
        ('side_order', ctypes.c_void_p * 2), ('side_n', ctypes.c_int64 * 2),
    ]


COMM_ID_BYTES = 128          # TPE_COMM_ID_BYTES
EXCHANGE_HEADER = 64         # TPE_EXCHANGE_HEADER
GATHER_FN = ctypes.CFUNCTYPE(ctypes.c_int, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_int64, ctypes.c_void_p)


class Exchange(ctypes.Structure):
    """tpe_exchange: the candidate-shard exchange of a sharded tpe_suggest_tree."""
    _fields_ = [
        ('rank', ctypes.c_int32), ('world', ctypes.c_int32), ('comm', ctypes.c_void_p),
        ('gather', GATHER_FN), ('ctx', ctypes.c_void_p), ('dev', ctypes.c_void_p), ('dev_bytes', ctypes.c_int64),
        ('always', ctypes.c_int32), ('reserved', ctypes.c_int32),
    ]


TREE_LABEL_DTYPE = np.dtype(dict(
    names=[f for f, _ in TreeLabel._fields_],
    formats=['<i4', '<i4', '<i4', '<i4', '<f8', '<f8', '<f8', '<f8', '<u8', '<u8', '<u8', '<u8', '<i8', '<i4', '<i4',
             ('<i4', (TREE_MAX_PARENTS,)), ('<i4', (TREE_MAX_PARENTS,)), '<f8', ('<u8', (2,)), ('<u8', (2,)),
             ('<u8', (2,)), ('<i8', (2,)), '<u8', '<u8', '<u8', '<i8', '<u8', '<u8', ('<u8', (2,)), ('<i8', (2,))],
    offsets=[getattr(TreeLabel, f).offset for f, _ in TreeLabel._fields_], itemsize=ctypes.sizeof(TreeLabel)))

EXPORTS = ('tpe_abi_version', 'tpe_last_error', 'tpe_device_count', 'tpe_tile_size', 'tpe_pinned_device_address',
           'tpe_sort_workspace_bytes', 'tpe_run_batch', 'tpe_fit_above', 'tpe_tables',
           'tpe_sample', 'tpe_sort', 'tpe_score_above', 'tpe_finalize', 'tpe_select', 'tpe_host_fit_parzen', 'tpe_host_fit_split',
           'tpe_host_cat_probs', 'tpe_host_cat_split', 'tpe_host_pack_level', 'tpe_level_run',
           'tpe_replay_mixture', 'tpe_replay_categorical', 'tpe_level_profile', 'tpe_level_profile_read',
           'tpe_suggest_tree', 'tpe_comm_unique_id', 'tpe_comm_init', 'tpe_comm_destroy', 'tpe_combine_results',
           'tpe_host_threads', 'tpe_host_phases', 'tpe_exchange_allgather', 'tpe_debug_fast_lg',
           'tpe_collectives_issued', 'tpe_level_resident', 'tpe_level_resident_fused', 'tpe_scatter_f64', 'tpe_move_ranges', 'tpe_report_scratch_bytes', 'tpe_report',
           'tpe_report_profile', 'tpe_joint_scratch_bytes', 'tpe_joint_run', 'tpe_joint_profile',
           'tpe_joint_mixed_run', 'tpe_joint_quant_table_bytes', 'tpe_joint_quant_run', 'tpe_joint_quant_profile',
           'tpe_joint_wide_scratch_bytes', 'tpe_joint_wide_run', 'tpe_joint_wide_profile',
           'tpe_joint_wide_mixed_scratch_bytes', 'tpe_joint_wide_mixed_run',
           'tpe_joint_wide_quant_scratch_bytes', 'tpe_joint_wide_quant_run', 'tpe_joint_wide_quant_profile',
           'tpe_joint_seg_scratch_bytes', 'tpe_joint_seg_run', 'tpe_joint_mseg_scratch_bytes',
           'tpe_joint_mseg_table_bytes', 'tpe_joint_mseg_run', 'tpe_joint_wide_seg_scratch_bytes',
           'tpe_joint_wide_seg_run', 'tpe_joint_report_scratch_bytes',
           'tpe_joint_report', 'tpe_joint_report_profile', 'tpe_joint_run_shard', 'tpe_joint_liar_scratch_bytes',
           'tpe_joint_liar', 'tpe_joint_liar_mixed_scratch_bytes', 'tpe_joint_liar_mixed',
           'tpe_joint_liar_seg_scratch_bytes', 'tpe_joint_liar_seg', 'tpe_joint_liar_mseg_scratch_bytes',
           'tpe_joint_liar_mseg')

# host phases of tpe_suggest_tree (tpe_host_phases order)
PHASES = ('prefit', 'pack', 'launched', 'synced', 'level', 'return', 'recs')

# tpe_level_run stages (tpe_level_profile_read order)
STAGES = ('fit', 'k_tables', 'k_sample', 'sort', 'above', 'k_finalize', 'k_select')


class StageProf(ctypes.Structure):
    """tpe_stage_prof: one stage of the last profiled tpe_level_run."""
    _fields_ = [('ms', ctypes.c_double), ('units', ctypes.c_double), ('ce', ctypes.c_double),
                ('launches', ctypes.c_int32), ('kernel_ns', ctypes.c_int32)]


class MTState(ctypes.Structure):
    """tpe_mt_state: numpy's legacy RandomState (MT19937 key, position and the
    cached polar-method gauss)."""
    _fields_ = [('key', ctypes.c_uint32 * 624), ('pos', ctypes.c_int32), ('has_gauss', ctypes.c_int32),
                ('gauss', ctypes.c_double)]


class NativeUnavailable(RuntimeError):
    """libtpe_hip.so is missing, fails to load, or finds no HIP device."""


_LIB = None


def load(path=LIB_PATH):
    """Load (once) and type the C-ABI.  Raises NativeUnavailable, never falls back."""
    global _LIB
    if _LIB is not None:
        return _LIB
    if not os.path.exists(path):
        raise NativeUnavailable('%s is not built (run __graft_entry__.build() or '
                                'python -m hyperopt_amd.build)' % path)
    try:
        lib = ctypes.CDLL(path)
    except OSError as e:
        raise NativeUnavailable('cannot load %s: %s' % (path, e))
    lib.tpe_abi_version.restype = ctypes.c_int
    lib.tpe_last_error.restype = ctypes.c_char_p
    lib.tpe_device_count.argtypes = [ctypes.POINTER(ctypes.c_int)]
    lib.tpe_tile_size.restype = ctypes.c_int
    lib.tpe_pinned_device_address.argtypes = [ctypes.c_void_p, ctypes.POINTER(ctypes.c_void_p)]
    lib.tpe_pinned_device_address.restype = ctypes.c_int
    lib.tpe_sort_workspace_bytes.argtypes = [ctypes.c_int64, ctypes.POINTER(ctypes.c_uint64)]
    lib.tpe_sort_workspace_bytes.restype = ctypes.c_int
    for name in ('tpe_run_batch', 'tpe_fit_above', 'tpe_tables', 'tpe_sample', 'tpe_sort', 'tpe_score_above', 'tpe_finalize', 'tpe_select'):
        fn = getattr(lib, name)
        fn.argtypes = [ctypes.POINTER(Batch), ctypes.c_void_p]
        fn.restype = ctypes.c_int
    P = ctypes.c_void_p
    lib.tpe_host_fit_parzen.argtypes = [P, ctypes.c_int64, P, ctypes.c_double, ctypes.c_double, ctypes.c_double,
                                        ctypes.c_int32, P, P, P]
    lib.tpe_host_fit_parzen.restype = ctypes.c_int64
    D = ctypes.c_double
    lib.tpe_host_fit_split.argtypes = [P, P, P, ctypes.c_int64, P, ctypes.c_int64, D, D, D, ctypes.c_int32, P, P]
    lib.tpe_host_fit_split.restype = ctypes.c_int
    lib.tpe_host_cat_probs.argtypes = [P, ctypes.c_int64, ctypes.c_int32, P, ctypes.c_double, ctypes.c_int32, P]
    lib.tpe_host_cat_probs.restype = ctypes.c_int
    lib.tpe_host_cat_split.argtypes = [P, P, ctypes.c_int64, P, ctypes.c_int64, ctypes.c_int32, P, D, ctypes.c_int32,
                                       P, P]
    lib.tpe_host_cat_split.restype = ctypes.c_int
    I64 = ctypes.c_int64
    lib.tpe_replay_mixture.argtypes = [P, P, P, P, I64, ctypes.c_int32, D, D, I64, P]
    lib.tpe_replay_mixture.restype = ctypes.c_int
    lib.tpe_replay_categorical.argtypes = [P, P, I64, I64, P]
    lib.tpe_replay_categorical.restype = ctypes.c_int
    lib.tpe_host_pack_level.argtypes = [ctypes.c_void_p, ctypes.c_int32, ctypes.c_int32, ctypes.c_uint64,
                                        ctypes.c_int64, ctypes.c_int64, ctypes.c_int32, P, ctypes.c_int64,
                                        ctypes.POINTER(PackInfo)]
    lib.tpe_host_pack_level.restype = ctypes.c_int
    lib.tpe_level_run.argtypes = [ctypes.c_void_p, ctypes.c_int32, ctypes.c_int32, ctypes.c_uint64,
                                  ctypes.c_int64, ctypes.c_int64, ctypes.c_int32, ctypes.c_int32, ctypes.POINTER(LevelWS),
                                  ctypes.POINTER(LevelNeed), P, P]
    lib.tpe_level_run.restype = ctypes.c_int
    I32 = ctypes.c_int32
    lib.tpe_suggest_tree.argtypes = [P, I32, P, I64, D, I32, P, I32, I32, I64, I64, ctypes.POINTER(Exchange),
                                     ctypes.c_uint64, D, I64, I32,
                                     ctypes.POINTER(LevelWS), ctypes.POINTER(LevelNeed), P, P, P, P, P]
    lib.tpe_suggest_tree.restype = ctypes.c_int
    lib.tpe_comm_unique_id.argtypes = [P]
    lib.tpe_comm_unique_id.restype = ctypes.c_int
    lib.tpe_comm_init.argtypes = [I32, I32, P, I32, ctypes.POINTER(ctypes.c_void_p)]
    lib.tpe_comm_init.restype = ctypes.c_int
    lib.tpe_comm_destroy.argtypes = [P]
    lib.tpe_comm_destroy.restype = ctypes.c_int
    lib.tpe_combine_results.argtypes = [P, I32, I64, P]
    lib.tpe_combine_results.restype = ctypes.c_int
    lib.tpe_exchange_allgather.argtypes = [ctypes.POINTER(Exchange), P, I64, P, P]
    lib.tpe_exchange_allgather.restype = ctypes.c_int
    lib.tpe_host_threads.argtypes = [I32, ctypes.POINTER(I32)]
    lib.tpe_host_threads.restype = ctypes.c_int
    lib.tpe_host_phases.argtypes = [I32, P, I32]
    lib.tpe_host_phases.restype = ctypes.c_int
    lib.tpe_debug_fast_lg.argtypes = [P, I64]
    lib.tpe_debug_fast_lg.restype = ctypes.c_int
    lib.tpe_level_resident.argtypes = [I32, ctypes.POINTER(I64)]
    lib.tpe_level_resident.restype = ctypes.c_int
    lib.tpe_level_resident_fused.argtypes = [ctypes.POINTER(I64)]
    lib.tpe_level_resident_fused.restype = ctypes.c_int
    lib.tpe_collectives_issued.argtypes = [ctypes.POINTER(I64)]
    lib.tpe_collectives_issued.restype = ctypes.c_int
    lib.tpe_scatter_f64.argtypes = [P, I64, P, P]
    lib.tpe_scatter_f64.restype = ctypes.c_int
    lib.tpe_move_ranges.argtypes = [P, ctypes.c_int32, ctypes.c_int32, P, P, P]
    lib.tpe_move_ranges.restype = ctypes.c_int
    lib.tpe_report_scratch_bytes.argtypes = [I64, I32, ctypes.POINTER(ctypes.c_uint64)]
    lib.tpe_report_scratch_bytes.restype = ctypes.c_int
    lib.tpe_report.argtypes = [ctypes.POINTER(Batch), I32, P, P, P, P, ctypes.c_uint64, P]
    lib.tpe_report.restype = ctypes.c_int
    lib.tpe_report_profile.argtypes = [I32, P]
    lib.tpe_report_profile.restype = ctypes.c_int
    lib.tpe_joint_scratch_bytes.argtypes = [I32, I32, ctypes.POINTER(ctypes.c_uint64)]
    lib.tpe_joint_scratch_bytes.restype = ctypes.c_int
    lib.tpe_joint_run.argtypes = [ctypes.POINTER(JointArgs), P, P, P, P, P, ctypes.c_uint64, P]
    lib.tpe_joint_run.restype = ctypes.c_int
    lib.tpe_joint_mixed_run.argtypes = [ctypes.POINTER(JointMixedArgs), P, P, P, P, P, ctypes.c_uint64, P]
    lib.tpe_joint_mixed_run.restype = ctypes.c_int
    lib.tpe_joint_quant_table_bytes.argtypes = [I32, I32, I32, ctypes.POINTER(ctypes.c_uint64)]
    lib.tpe_joint_quant_table_bytes.restype = ctypes.c_int
    lib.tpe_joint_quant_run.argtypes = [ctypes.POINTER(JointQuantArgs), P, P, P, P, P, ctypes.c_uint64, P]
    lib.tpe_joint_quant_run.restype = ctypes.c_int
    lib.tpe_joint_quant_profile.argtypes = [P]
    lib.tpe_joint_quant_profile.restype = ctypes.c_int
    lib.tpe_joint_wide_scratch_bytes.argtypes = [I32, I32, I32, ctypes.POINTER(ctypes.c_uint64)]
    lib.tpe_joint_wide_scratch_bytes.restype = ctypes.c_int
    lib.tpe_joint_wide_run.argtypes = [ctypes.POINTER(JointWideArgs), P, P, P, P, P, ctypes.c_uint64, P]
    lib.tpe_joint_wide_run.restype = ctypes.c_int
    lib.tpe_joint_wide_profile.argtypes = [P]
    lib.tpe_joint_wide_profile.restype = ctypes.c_int
    lib.tpe_joint_wide_mixed_scratch_bytes.argtypes = [I32, I32, I32, I32, ctypes.POINTER(ctypes.c_uint64)]
    lib.tpe_joint_wide_mixed_scratch_bytes.restype = ctypes.c_int
    lib.tpe_joint_wide_mixed_run.argtypes = [ctypes.POINTER(JointWideMixedArgs), P, P, P, P, P, ctypes.c_uint64, P]
    lib.tpe_joint_wide_mixed_run.restype = ctypes.c_int
    lib.tpe_joint_wide_quant_scratch_bytes.argtypes = [I32, I32, I32, I32, I32, ctypes.POINTER(ctypes.c_uint64)]
    lib.tpe_joint_wide_quant_scratch_bytes.restype = ctypes.c_int
    lib.tpe_joint_wide_quant_run.argtypes = [ctypes.POINTER(JointWideQuantArgs), P, P, P, P, P, ctypes.c_uint64, P]
    lib.tpe_joint_wide_quant_run.restype = ctypes.c_int
    lib.tpe_joint_wide_quant_profile.argtypes = [P]
    lib.tpe_joint_wide_quant_profile.restype = ctypes.c_int
    lib.tpe_joint_seg_scratch_bytes.argtypes = [I32, I32, ctypes.POINTER(ctypes.c_uint64)]
    lib.tpe_joint_seg_scratch_bytes.restype = ctypes.c_int
    lib.tpe_joint_seg_run.argtypes = [ctypes.POINTER(JointSegArgs), P, P, P, P, P, ctypes.c_uint64, P]
    lib.tpe_joint_seg_run.restype = ctypes.c_int
    lib.tpe_joint_wide_seg_scratch_bytes.argtypes = [I32, I32, ctypes.POINTER(ctypes.c_uint64)]
    lib.tpe_joint_wide_seg_scratch_bytes.restype = ctypes.c_int
    lib.tpe_joint_wide_seg_run.argtypes = [ctypes.POINTER(JointWideSegArgs), P, P, P, P, P, ctypes.c_uint64, P]
    lib.tpe_joint_wide_seg_run.restype = ctypes.c_int
    lib.tpe_joint_mseg_scratch_bytes.argtypes = [I32, I32, ctypes.POINTER(ctypes.c_uint64)]
    lib.tpe_joint_mseg_scratch_bytes.restype = ctypes.c_int
    lib.tpe_joint_mseg_table_bytes.argtypes = [P, I32, ctypes.POINTER(ctypes.c_uint64)]
    lib.tpe_joint_mseg_table_bytes.restype = ctypes.c_int
    lib.tpe_joint_mseg_run.argtypes = [ctypes.POINTER(JointMSegArgs), P, P, P, P, P, ctypes.c_uint64, P]
    lib.tpe_joint_mseg_run.restype = ctypes.c_int
    lib.tpe_joint_run_shard.argtypes = [I32, P, ctypes.POINTER(JointShard), P, P, P, P, P, ctypes.c_uint64, P]
    lib.tpe_joint_run_shard.restype = ctypes.c_int
    lib.tpe_joint_report_scratch_bytes.argtypes = [I32, I32, I32, ctypes.POINTER(ctypes.c_uint64)]
    lib.tpe_joint_report_scratch_bytes.restype = ctypes.c_int
    lib.tpe_joint_report.argtypes = [ctypes.POINTER(JointReportArgs), I32, P, P, P, P, P, ctypes.c_uint64, P]
    lib.tpe_joint_report.restype = ctypes.c_int
    lib.tpe_joint_report_profile.argtypes = [I32, P]
    lib.tpe_joint_report_profile.restype = ctypes.c_int
    lib.tpe_joint_liar_scratch_bytes.argtypes = [I32, I32, I32, I32, ctypes.POINTER(ctypes.c_uint64)]
    lib.tpe_joint_liar_scratch_bytes.restype = ctypes.c_int
    lib.tpe_joint_liar.argtypes = [ctypes.POINTER(JointLiarArgs), P, P, P, P, ctypes.c_uint64, P]
    lib.tpe_joint_liar.restype = ctypes.c_int
    lib.tpe_joint_liar_mixed_scratch_bytes.argtypes = [I32] * 7 + [ctypes.POINTER(ctypes.c_uint64)]
    lib.tpe_joint_liar_mixed_scratch_bytes.restype = ctypes.c_int
    lib.tpe_joint_liar_mixed.argtypes = [ctypes.POINTER(JointLiarMixedArgs), P, P, P, P, ctypes.c_uint64, P]
    lib.tpe_joint_liar_mixed.restype = ctypes.c_int
    lib.tpe_joint_liar_seg_scratch_bytes.argtypes = [P, I32, I32, ctypes.POINTER(ctypes.c_uint64)]
    lib.tpe_joint_liar_seg_scratch_bytes.restype = ctypes.c_int
    lib.tpe_joint_liar_seg.argtypes = [ctypes.POINTER(JointLiarSegArgs), P, P, P, P, ctypes.c_uint64, P]
    lib.tpe_joint_liar_seg.restype = ctypes.c_int
    lib.tpe_joint_liar_mseg_scratch_bytes.argtypes = [P, I32, I32, ctypes.POINTER(ctypes.c_uint64)]
    lib.tpe_joint_liar_mseg_scratch_bytes.restype = ctypes.c_int
    lib.tpe_joint_liar_mseg.argtypes = [ctypes.POINTER(JointLiarMSegArgs), P, P, P, P, ctypes.c_uint64, P]
    lib.tpe_joint_liar_mseg.restype = ctypes.c_int
    lib.tpe_joint_profile.argtypes = [I32, P]
    lib.tpe_joint_profile.restype = ctypes.c_int
    lib.tpe_level_profile.argtypes = [ctypes.c_int32]
    lib.tpe_level_profile.restype = ctypes.c_int
    lib.tpe_level_profile_read.argtypes = [ctypes.POINTER(StageProf), ctypes.c_int32]
    lib.tpe_level_profile_read.restype = ctypes.c_int
    if lib.tpe_abi_version() != ABI_VERSION:
        raise NativeUnavailable('ABI mismatch: library %d, bindings %d' % (lib.tpe_abi_version(), ABI_VERSION))
    _LIB = lib
    return lib


def check(rc, lib, what):
    if rc != 0:
        msg = lib.tpe_last_error().decode(errors='replace')
        raise RuntimeError('%s failed (%d): %s' % (what, rc, msg))


def report_chunks(n_problems, total_cand):
    """Chunk slots of a batch's candidate report (include/tpe_hip.h "Chunk
    slots"): n_problems * ceil(ceil(total_cand / n_problems) / TPE_REPORT_CHUNK)."""
    if n_problems <= 0 or total_cand <= 0:
        return 0
    per = -(-int(total_cand) // int(n_problems))
    return int(n_problems) * (-(-per // REPORT_CHUNK))


def tile_size():
    return load().tpe_tile_size()


def collectives_issued(lib=None):
    """ncclAllGather calls the library has issued in this process
    (tpe_collectives_issued)."""
    lib = lib or load()
    n = ctypes.c_int64(0)
    check(lib.tpe_collectives_issued(ctypes.byref(n)), lib, 'tpe_collectives_issued')
    return int(n.value)


def level_resident(mode=-1, lib=None):
    """tpe_level_resident: set the resident-level mode (0 off and drop, 1 on,
    2 drop only, < 0 query); returns (on, {hits, misses, fit_reuses, drops})."""
    lib = lib or load()
    st = (ctypes.c_int64 * 4)()
    on = lib.tpe_level_resident(int(mode), st)
    return bool(on), dict(zip(('hits', 'misses', 'fit_reuses', 'drops'), (int(v) for v in st)))


def level_resident_fused(lib=None):
    """tpe_level_resident_fused: {fused, fallbacks} — the hits that ran the
    argument-keyed sample kernel alone, and those of them whose host selection
    did not settle (the patch kernel behind it)."""
    lib = lib or load()
    st = (ctypes.c_int64 * 2)()
    check(lib.tpe_level_resident_fused(st), lib, 'tpe_level_resident_fused')
    return {'fused': int(st[0]), 'fallbacks': int(st[1])}
