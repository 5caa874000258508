"""Python binding (ctypes) of the C ABI in include/ibwa_aln.h.

This is plumbing for tests and bench.py; the product interface is the C ABI
and the `ibwa-amd aln` CLI.  Every call goes to libibwa_amd.so on a gfx950
device; there is no CPU path here -- if the library or the device is missing
the call raises.
"""
import ctypes
import os
import struct

import numpy as np

from . import _native

c = ctypes


class GapOpt(c.Structure):
    """gap_opt_t (bwtaln.h:105-115) == ibwa_gap_opt_t; also the 64-byte .sai header."""
    _fields_ = [(n, c.c_int) for n in ("s_mm", "s_gapo", "s_gape", "mode", "indel_end_skip",
                                       "max_del_occ", "max_entries")] + \
               [("fnr", c.c_float)] + \
               [(n, c.c_int) for n in ("max_diff", "max_gapo", "max_gape", "max_seed_diff",
                                       "seed_len", "n_threads", "max_top2", "trim_qual")]


class RunStats(c.Structure):
    _fields_ = [("ms_width", c.c_double), ("ms_search", c.c_double), ("ms_retry", c.c_double),
                ("ms_total", c.c_double), ("n_retry", c.c_int64), ("n_launch_width", c.c_int64),
                ("n_launch_search", c.c_int64), ("path", c.c_int), ("kmer_k", c.c_int),
                ("n_stack_overflow", c.c_int64), ("n_aln_overflow", c.c_int64), ("n_heavy", c.c_int64), ("ms_sw", c.c_double),
                ("n_coop", c.c_int64), ("ms_coop", c.c_double), ("ms_sa2pos", c.c_double),
                ("sa2pos_full", c.c_int), ("ms_coop_width", c.c_double), ("ms_coop_roots", c.c_double),
                ("n_resumed", c.c_int64), ("resume_records", c.c_int64),
                ("resume_records_peak", c.c_int64), ("resume_records_cap", c.c_int64),
                ("coop_pages_peak", c.c_int64), ("coop_pages_cap", c.c_int64), ("ms_alloc", c.c_double),
                ("n_tail_jumps", c.c_int64), ("n_width_tab_steps", c.c_int64),
                ("ms_bsw2_seed", c.c_double), ("n_bsw2_retry", c.c_int64), ("bsw2_arena_peak", c.c_int64),
                ("first_pass_lw", c.c_int), ("first_pass_block", c.c_int)]


class RefSeq(c.Structure):
    """bwa_seq_t (bwtaln.h:62-93) == ibwa_ref_seq_t (ibwa_bwa_compat.h)"""
    _fields_ = [("name", c.c_void_p), ("seq", c.c_void_p), ("rseq", c.c_void_p), ("qual", c.c_void_p),
                ("len", c.c_uint32, 20), ("strand", c.c_uint32, 1), ("type", c.c_uint32, 2),
                ("dummy", c.c_uint32, 1), ("extra_flag", c.c_uint32, 8),
                ("n_mm", c.c_uint32, 8), ("n_gapo", c.c_uint32, 8), ("n_gape", c.c_uint32, 8),
                ("mapQ", c.c_uint32, 8), ("score", c.c_int), ("clip_len", c.c_int), ("n_aln", c.c_int),
                ("aln", c.c_void_p), ("n_multi", c.c_int), ("multi", c.c_void_p), ("sa", c.c_uint32),
                ("pos", c.c_uint64), ("remapped_pos", c.c_uint64), ("dbidx", c.c_uint32),
                ("remapped_dbidx", c.c_uint32), ("remapped_seqid", c.c_int32), ("remap_identical", c.c_int),
                ("c1", c.c_uint64, 28), ("c2", c.c_uint64, 28), ("seQ", c.c_uint64, 8), ("n_cigar", c.c_int),
                ("cigar", c.c_void_p), ("tid", c.c_int), ("bc", c.c_char * 16),
                ("full_len", c.c_uint32, 20), ("nm", c.c_uint32, 12), ("md", c.c_void_p)]


class PeOpt(c.Structure):
    """pe_opt_t (bwtaln.h:120-128) == ibwa_ref_pe_opt_t"""
    _fields_ = [(n, c.c_int) for n in ("max_isize", "force_isize", "max_occ", "n_multi", "N_multi", "n_threads",
                                       "type", "is_sw", "is_preload", "remapping")] + [("ap_prior", c.c_double)]


class IsizeInfo(c.Structure):
    """isize_info_t (bwapair.h:8-11) == ibwa_ref_isize_info_t"""
    _fields_ = [("avg", c.c_double), ("std", c.c_double), ("ap_prior", c.c_double), ("low", c.c_uint32),
                ("high", c.c_uint32), ("high_bayesian", c.c_uint32)]


assert c.sizeof(GapOpt) == 64
ALN_DTYPE = np.dtype([("info", "<u4"), ("k", "<u4"), ("l", "<u4"), ("score", "<i4")])  # bwt_aln1_t

MODE_GAPE, MODE_COMPREAD, MODE_LOGGAP, MODE_NONSTOP = 0x01, 0x02, 0x04, 0x10
MODE_BAM, MODE_BAM_SE, MODE_BAM_READ1, MODE_BAM_READ2, MODE_IL13 = 0x20, 0x40, 0x80, 0x100, 0x200

# every exported symbol declared in include/ibwa_aln.h: name -> (restype, argtypes)
_vp, _i, _i64, _u32, _u64 = c.c_void_p, c.c_int, c.c_int64, c.c_uint32, c.c_uint64
CAPI = {
    "ibwa_last_error": (c.c_char_p, []),
    "ibwa_free": (None, [_vp]),
    "ibwa_gap_init_opt": (None, [c.POINTER(GapOpt)]),
    "ibwa_cal_maxdiff": (_i, [_i, c.c_double, c.c_double]),
    "ibwa_ctx_create": (_i, [_i, c.POINTER(_vp)]),
    "ibwa_device_count": (_i, [c.POINTER(_i)]),
    "ibwa_device_bytes": (_i, [c.POINTER(c.c_int64), c.POINTER(c.c_int64)]),
    "ibwa_device_memory": (_i, [_i, c.POINTER(c.c_uint64), c.POINTER(c.c_uint64)]),
    "ibwa_reserve": (_i, [_i, c.c_uint64]),
    "ibwa_arena_stats": (_i, [_i, c.POINTER(c.c_uint64), c.POINTER(c.c_uint64), c.POINTER(c.c_uint64)]),
    "ibwa_fq_parse": (_i, [_vp, _vp, c.c_uint64, _i, _i, c.POINTER(c.c_int64), c.POINTER(c.c_uint64), c.POINTER(_i),
                           _vp, _vp, c.c_int64]),
    "ibwa_fq_stats": (_i, [_vp, c.POINTER(c.c_int64), c.POINTER(c.c_double)]),
    "ibwa_fq_fetch": (_i, [_vp, c.c_int64, c.c_int64, _vp, _vp, _vp, c.c_uint64]),
    "ibwa_fq_offset": (_i,[_vp, c.c_int64, c.POINTER(c.c_uint64)]),
    "ibwa_fq_share_scratch": (_i, [_vp, _vp]),
    "ibwa_release": (_i, [_i]),
    "ibwa_batch_fetch_sai": (_i, [_vp, _vp, c.c_uint64, c.POINTER(c.c_uint64), c.POINTER(c.c_int64)]),
    "ibwa_batch_stage_fq": (_i, [_vp, _vp, c.c_int64, c.c_int64, _i]),
    "ibwa_host_alloc": (_i, [c.c_uint64, c.POINTER(_vp)]),
    "ibwa_host_free": (_i, [_vp]),
    "ibwa_ctx_destroy": (None, [_vp]),
    "ibwa_ctx_load_bwt": (_i, [_vp, _i, _u32, c.POINTER(_u32), _vp, _u64]),
    "ibwa_ctx_load_bwt_file": (_i, [_vp, _i, c.c_char_p]),
    "ibwa_ctx_clone_index": (_i, [_vp, _vp]),
    "ibwa_ctx_share_index": (_i, [_vp, _vp]),
    "ibwa_aln_batch": (_i, [_vp, c.POINTER(GapOpt), _i64, _vp, _vp, _vp, _i, _vp, c.POINTER(_vp),
                            c.POINTER(_i64)]),
    "ibwa_batch_stage": (_i, [_vp, _i64, _vp, _vp, _vp]),
    "ibwa_batch_run": (_i, [_vp, c.POINTER(GapOpt), _i]),
    "ibwa_batch_fetch": (_i, [_vp, _vp, c.POINTER(_vp), c.POINTER(_i64)]),
    "ibwa_batch_stats": (_i, [_vp, c.POINTER(RunStats)]),
    "ibwa_ctx_set_tuning": (_i, [_vp, _i, _i, _i]),
    "ibwa_aln_parse_args": (_i, [_i, c.POINTER(c.c_char_p), c.POINTER(GapOpt), c.POINTER(_i), c.POINTER(c.c_char_p)]),
    "ibwa_aln_parse_args2": (_i, [_i, c.POINTER(c.c_char_p), c.POINTER(GapOpt), c.POINTER(_i), c.POINTER(c.c_char_p),
                                  c.POINTER(c.c_char_p)]),
    "ibwa_batch_retry_info": (_i, [_vp, _vp, _vp, _i64, c.POINTER(_i64)]),
    "ibwa_batch_diag": (_i, [_vp, _i, _vp, _u64]),
    "ibwa_ctx_set_option": (_i, [_vp, c.c_char_p, c.c_long]),
    "ibwa_build_id": (c.c_char_p, []),
    "ibwa_occ4": (_i, [_vp, _i, _i64, _vp, _vp]),
    "ibwa_ctx_load_sa": (_i, [_vp, _i, _u32, _vp, _u64]),
    "ibwa_ctx_load_sa_file": (_i, [_vp, _i, c.c_char_p]),
    "ibwa_ctx_expand_sa": (_i, [_vp]),
    "ibwa_ctx_prepare": (_i, [_vp, c.POINTER(GapOpt)]),
    "ibwa_ctx_derive_sa": (_i, [_vp, _u32]),
    "ibwa_sa2pos": (_i, [_vp, _i64, _vp, _vp, _vp, _u64, _vp]),
    "ibwa_ctx_build_index": (_i, [_vp, _vp, _u64, _i]),
    "ibwa_ctx_bwt_info": (_i, [_vp, _i, c.POINTER(_u32), c.POINTER(_u32), c.POINTER(_u64)]),
    "ibwa_ctx_export_bwt": (_i, [_vp, _i, _vp, _u64]),
    "ibwa_ctx_export_sa": (_i, [_vp, _i, _vp, _u64]),
    "ibwa_ctx_build_rounds": (_i, [_vp, _i, c.POINTER(_i)]),
    "ibwa_sw_batch": (_i, [_vp, _i64, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, c.POINTER(c.c_void_p),
                           c.POINTER(_i64)]),
    "ibwa_global_batch": (_i, [_vp, _i64, _vp, _vp, _vp, _vp, _vp, _vp, _i, _i, _vp, _vp, _vp, c.POINTER(c.c_void_p),
                               c.POINTER(_i64)]),
    "ibwa_paired_sw": (_i, [_vp, _i, c.POINTER(c.POINTER(RefSeq)), c.POINTER(PeOpt), c.POINTER(IsizeInfo), _vp,
                            _u64, c.POINTER(_u64), c.POINTER(_u64)]),
    "ibwa_paired_sw_dbs": (_i, [_vp, _i, c.POINTER(c.POINTER(RefSeq)), c.POINTER(PeOpt), c.POINTER(IsizeInfo), _i, _vp,
                                _vp, _vp, c.POINTER(_u64), c.POINTER(_u64)]),
    "ibwa_sw_core_batch": (_i, [_vp, _i64, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _i64, _vp, _vp,
                                c.POINTER(c.c_void_p)]),
    "ibwa_aln_param_preset": (_i, [c.c_char_p, _vp]),
    "ibwa_stdaln_batch": (_i, [_vp, _vp, _i, _i, _i64, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp,
                               c.POINTER(c.c_void_p), c.POINTER(_i64)]),
    "ibwa_stdaln_check": (_i, [_vp, _i, _i, _i64, _vp, _vp, _vp, _vp, _vp, _vp]),
    "ibwa_stdaln_chunks": (_i, [_vp, c.POINTER(_i64), c.POINTER(c.c_double)]),
    "ibwa_extend_batch": (_i, [_vp, _vp, _i, _i64, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp,
                               c.POINTER(c.c_void_p), c.POINTER(_i64)]),
    "ibwa_extend_check": (_i, [_vp, _i, _i64, _vp, _vp, _vp, _vp, _vp, _vp, _vp]),
    "ibwa_extend_seeds": (_i, [_vp, _vp, _i64, _vp, _vp, _vp, _i, _vp, _vp, _vp, _vp, _vp, _vp]),
    "ibwa_extend_stats": (_i, [_vp, c.POINTER(_i64)]),
    "ibwa_bsw2_opt_preset": (_i, [c.c_char_p, _vp]),
    "ibwa_bsw2_seed_batch": (_i, [_vp, _vp, _i64, _vp, _vp, _vp, _vp, _vp, _vp, c.POINTER(c.c_void_p), c.POINTER(_i64)]),
    "ibwa_bsw2_seed_check": (_i, [_vp, _i64, _vp, _vp, _vp, _vp]),
    "ibwa_bsw2_opt_for_len": (None, [_vp, _u32, c.POINTER(c.c_int32), c.POINTER(c.c_int32)]),
    "ibwa_bsw2_seed_stats": (_i, [_vp, c.POINTER(c.c_int64 * 8)]),
    "ibwa_bsw2_aln_opt_preset": (_i, [c.c_char_p, _vp]),
    "ibwa_bsw2_aln1_batch": (_i, [_vp, _vp, _i64, _vp, _vp, _vp, _vp, _vp, _vp, c.POINTER(c.c_void_p), c.POINTER(_i64)]),
    "ibwa_bsw2_extend_left_batch": (_i, [_vp, _vp, _i64, _vp, _vp, _vp, _vp, _vp, _vp, _vp]),
    "ibwa_bsw2_aln1_check": (_i, [_vp, _i64, _vp, _vp, _vp, _vp, _vp]),
    "ibwa_bsw2_aln1_stats": (_i, [_vp, c.POINTER(c.c_int64 * 8)]),
    "ibwa_ctx_load_pac": (_i, [_vp, _i, c.POINTER(_vp), c.POINTER(_u64)]),
    "ibwa_pac_extract": (_i, [_vp, _i64, _vp, _vp, _vp, _vp, _vp]),
    "ibwa_refine_batch": (_i, [_vp, _i64, _vp, _vp, _vp, _vp, _vp, _vp, _vp, c.POINTER(c.c_void_p), c.POINTER(_i64)]),
    "ibwa_md_batch": (_i, [_vp, _i64, _vp, _vp, _vp, _vp, _vp, _vp, _vp, c.POINTER(c.c_void_p), c.POINTER(c.c_void_p)]),
    "ibwa_pac2cspac": (_i, [_vp, _vp, _u64, _vp]),
    "ibwa_ctx_load_ntpac": (_i, [_vp, _i, c.POINTER(_vp), c.POINTER(_u64)]),
    "ibwa_cs2nt_rows": (_i, [_vp, _i64, _vp, _vp, _vp, _vp, _vp, _vp]),
    "ibwa_cs2nt_batch": (_i, [_vp, _i64, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp]),
}


def declare(L):
    import os
    older = bool(os.environ.get("IBWA_LIB"))  # an A/B build (tools/) may predate newer entry points
    for name, (res, args) in CAPI.items():
        if older and not hasattr(L, name):
            continue
        f = getattr(L, name)
        f.restype = res
        f.argtypes = args


_declared = False


def lib():
    global _declared
    L = _native.lib()
    if not _declared:
        declare(L)
        _declared = True
    return L


class IbwaError(RuntimeError):
    pass


def _chk(rc):
    if rc != 0:
        raise IbwaError(f"ibwa error {rc}: {lib().ibwa_last_error().decode()}")


class AlnParam(c.Structure):
    """AlnParam (stdaln.h) == ibwa_aln_param_t"""
    _fields_ = [("gap_open", c.c_int), ("gap_ext", c.c_int), ("gap_end", c.c_int), ("matrix", c.POINTER(c.c_int32)),
                ("row", c.c_int), ("band_width", c.c_int)]


def aln_param(name):
    """The preset "blast", "aa2aa" or "bwa" (ibwa_aln_param_preset) as a dict with the keys gap_open,
    gap_ext, gap_end, matrix (row x row int32 array), row and band_width."""
    ap = AlnParam()
    _chk(lib().ibwa_aln_param_preset(name.encode(), c.byref(ap)))
    mat = np.ctypeslib.as_array(ap.matrix, shape=(ap.row, ap.row)).astype(np.int32)
    return {"gap_open": ap.gap_open, "gap_ext": ap.gap_ext, "gap_end": ap.gap_end, "matrix": mat, "row": ap.row,
            "band_width": ap.band_width}


def _aln_param_struct(param):
    """dict / (gap_open, gap_ext, gap_end, matrix, row, band_width) tuple / preset name -> (AlnParam, matrix)."""
    if isinstance(param, str):
        param = aln_param(param)
    if isinstance(param, dict):
        param = (param["gap_open"], param["gap_ext"], param["gap_end"], param["matrix"],
                 param.get("row"), param.get("band_width", 0))
    go, ge, gend, mat, row, band = param
    mat = np.ascontiguousarray(mat, dtype=np.int32)
    if row is None:
        row = int(round(mat.size ** 0.5))
    if mat.size != row * row:
        raise IbwaError(f"score matrix of {mat.size} entries for row {row}")
    ap = AlnParam(int(go), int(ge), int(gend), mat.ctypes.data_as(c.POINTER(c.c_int32)), int(row), int(band))
    return ap, mat


def _pair_arrays(seq1s, seq2s):
    n = len(seq1s)
    o1 = np.zeros(n, np.uint64)
    o2 = np.zeros(n, np.uint64)
    l1 = np.array([len(x) for x in seq1s], np.uint32)
    l2 = np.array([len(x) for x in seq2s], np.uint32)
    if n:
        o1[1:] = np.cumsum(l1[:-1])
        o2[1:] = np.cumsum(l2[:-1])
    s1 = np.concatenate([np.asarray(x, np.uint8) for x in seq1s] + [np.zeros(1, np.uint8)])
    s2 = np.concatenate([np.asarray(x, np.uint8) for x in seq2s] + [np.zeros(1, np.uint8)])
    return n, s1, o1, l1, s2, o2, l2


class Bsw2Opt(c.Structure):
    """ibwa_bsw2_opt_t: what bsw2_aln receives (t and coef scaled by a), and whether t and bw follow the read length."""
    _fields_ = [(n, c.c_int32) for n in ("a", "b", "q", "r", "t", "bw", "z", "is_")] + \
               [("coef", c.c_float), ("adjust", c.c_int32)]


BSW2_HIT_DTYPE = np.dtype([("k", "<u4"), ("l", "<u4"), ("flag", "<u4"), ("len", "<i4"), ("G", "<i4"), ("G2", "<i4"),
                           ("beg", "<i4"), ("end", "<i4")])  # ibwa_bsw2_hit_t
BSW2_MAX_LEN = 8192


def bsw2_opt(opt="bwasw", adjust=None, **kw):
    """A preset name ("bwasw": bsw2_init_opt's defaults), a dict with the keys a b q r t bw z is coef
    (missing ones from the preset) or a Bsw2Opt -> Bsw2Opt; keywords override, `is` spelled is_ or is."""
    if isinstance(opt, Bsw2Opt):
        o = Bsw2Opt.from_buffer_copy(opt)
    else:
        o = Bsw2Opt()
        _chk(lib().ibwa_bsw2_opt_preset((opt if isinstance(opt, str) else "bwasw").encode(), c.byref(o)))
        if isinstance(opt, dict):
            kw = dict(opt, **kw)
    for k, v in kw.items():
        setattr(o, "is_" if k == "is" else k, v)
    if adjust is not None:
        o.adjust = 1 if adjust else 0
    return o


class Bsw2AlnOpt(c.Structure):
    """ibwa_bsw2_aln_opt_t: the seeding's options, then bsw2opt_t's t_seeds and mask_level."""
    _fields_ = [("seed", Bsw2Opt), ("t_seeds", c.c_int32), ("mask_level", c.c_float)]


BSW2_ALN_HIT_DTYPE = np.dtype([("k", "<u4"), ("l", "<u4"), ("flag", "<u4"), ("n_seeds", "<u4"), ("len", "<i4"), ("G", "<i4"),
                               ("G2", "<i4"), ("beg", "<i4"), ("end", "<i4")])  # ibwa_bsw2_aln_hit_t


def bsw2_aln_opt(opt="bwasw", adjust=None, **kw):
    """As bsw2_opt, with the keys t_seeds and mask_level besides ("bwasw": 5 and 0.50) -> Bsw2AlnOpt."""
    if isinstance(opt, Bsw2AlnOpt):
        o = Bsw2AlnOpt.from_buffer_copy(opt)
        opt = o.seed
    else:
        o = Bsw2AlnOpt()
        _chk(lib().ibwa_bsw2_aln_opt_preset((opt if isinstance(opt, str) else "bwasw").encode(), c.byref(o)))
        if isinstance(opt, dict):
            kw = dict(opt, **kw)
            opt = "bwasw"
    for k in ("t_seeds", "mask_level"):
        if k in kw:
            setattr(o, k, kw.pop(k))
    o.seed = bsw2_opt(opt, adjust, **kw)
    return o


def bsw2_aln1_check(seqs, is_rev, opt="bwasw", adjust=None, u=None):
    """The checks of ibwa_bsw2_aln1_batch alone (no device): raises IbwaError on a refusal."""
    o = bsw2_aln_opt(opt, adjust)
    s, off, ln = Engine._pack_reads(seqs)
    rv = np.ascontiguousarray(is_rev, dtype=np.uint8)
    uu = None if u is None else np.ascontiguousarray(u, dtype=np.float64)
    if rv.size != ln.size or (uu is not None and uu.size != ln.size):
        raise IbwaError("bsw2 aln1: seqs, is_rev and u differ in length")
    _chk(lib().ibwa_bsw2_aln1_check(c.byref(o), ln.size, s.ctypes.data, off.ctypes.data, ln.ctypes.data, rv.ctypes.data,
                                    None if uu is None else uu.ctypes.data))


def bsw2_opt_for_len(opt, length):
    """(t, bw) of a read of that length, bwtsw2_aux.c:483-497."""
    o = bsw2_opt(opt)
    t, bw = c.c_int32(), c.c_int32()
    lib().ibwa_bsw2_opt_for_len(c.byref(o), int(length), c.byref(t), c.byref(bw))
    return t.value, bw.value


def bsw2_seed_check(seqs, strands, opt="bwasw", adjust=None):
    """The checks of ibwa_bsw2_seed_batch alone (no device): raises IbwaError on a refusal."""
    o = bsw2_opt(opt, adjust)
    s, off, ln = Engine._pack_reads(seqs)
    st = np.ascontiguousarray(strands, dtype=np.uint8)
    if st.size != ln.size:
        raise IbwaError("bsw2 seed: seqs and strands differ in length")
    _chk(lib().ibwa_bsw2_seed_check(c.byref(o), ln.size, s.ctypes.data, off.ctypes.data, ln.ctypes.data, st.ctypes.data))


_STDALN_TYPES = {"local": 0, "global": 1, "extend": 2}
_EXTEND_MODES = {"score": 0, "end": 1, "path": 2}


def stdaln_check(seq1s, seq2s, param, mode="local", thres=1):
    """The checks of ibwa_stdaln_batch alone (no device): raises IbwaError on a refusal."""
    ap, _mat = _aln_param_struct(param)
    n, s1, o1, l1, s2, o2, l2 = _pair_arrays(seq1s, seq2s)
    _chk(lib().ibwa_stdaln_check(c.byref(ap), _STDALN_TYPES[mode], thres, n, s1.ctypes.data, o1.ctypes.data,
                                 l1.ctypes.data, s2.ctypes.data, o2.ctypes.data, l2.ctypes.data))


def _g0_array(g0, n):
    """One G0 for every pair or one per pair -> int32[n] (None: the library's default of 1)."""
    if g0 is None:
        return None
    a = np.ascontiguousarray(np.broadcast_to(np.asarray(g0, dtype=np.int64), (n,)))
    if a.size and (a.min() < -2**31 or a.max() >= 2**31):
        raise IbwaError("extend: a G0 does not fit 32 bits")
    return a.astype(np.int32)


def extend_check(seq1s, seq2s, param, g0=1, mode="end"):
    """The checks of ibwa_extend_batch alone (no device): raises IbwaError on a refusal."""
    ap, _mat = _aln_param_struct(param)
    n, s1, o1, l1, s2, o2, l2 = _pair_arrays(seq1s, seq2s)
    g = _g0_array(g0, n)
    _chk(lib().ibwa_extend_check(c.byref(ap), _EXTEND_MODES[mode], n, s1.ctypes.data, o1.ctypes.data, l1.ctypes.data,
                                 s2.ctypes.data, o2.ctypes.data, l2.ctypes.data, None if g is None else g.ctypes.data))


def default_opt():
    o = GapOpt()
    lib().ibwa_gap_init_opt(c.byref(o))
    return o


def parse_aln_args(args):
    """The product's own `aln` option parser (ibwa_aln_parse_args: bwtaln.c:249-284) -> GapOpt."""
    argv = [b"aln"] + [a.encode() for a in args]
    arr = (c.c_char_p * len(argv))(*argv)
    o = GapOpt()
    rc = lib().ibwa_aln_parse_args(len(argv), arr, c.byref(o), None, None)
    if rc < 0:
        raise IbwaError(f"bad aln options {args}")
    if rc != len(argv):
        raise IbwaError(f"unexpected positional arguments in {args}")
    return o


def parse_aln_cmdline(args):
    """A whole `aln` command line (ibwa_aln_parse_args2: options, -G, -f, and -F of the pair mode)
    -> (GapOpt, n_gpus, fn_out, fn_out2, first_positional); the paths are None when not given and
    first_positional indexes `args` (len(args) when there is no positional argument; options come
    before the positional arguments, as on the CLI)."""
    argv = [b"aln"] + [a.encode() for a in args]
    arr = (c.c_char_p * len(argv))(*argv)
    o, n_gpus, f1, f2 = GapOpt(), _i(1), c.c_char_p(), c.c_char_p()
    rc = lib().ibwa_aln_parse_args2(len(argv), arr, c.byref(o), c.byref(n_gpus), c.byref(f1), c.byref(f2))
    if rc < 0:
        raise IbwaError(f"bad aln options {args}")
    paths = [p.value.decode() if p.value is not None else None for p in (f1, f2)]
    return o, n_gpus.value, paths[0], paths[1], rc - 1


def read_bwt_file(path):
    """bwt_restore_bwt (bwtio.c:51-70): -> (primary, L2[1..4], words uint32)."""
    with open(path, "rb") as f:
        primary, = struct.unpack("<I", f.read(4))
        L2 = struct.unpack("<4I", f.read(16))
        words = np.frombuffer(f.read(), dtype=np.uint32)
    return primary, L2, words


class Engine:
    """One device context (one GPU) with both FM-indexes resident in HBM."""

    def __init__(self, device=0):
        L = lib()
        h = c.c_void_p()
        _chk(L.ibwa_ctx_create(device, c.byref(h)))
        self.h = h
        self.device = device

    def close(self):
        if self.h:
            lib().ibwa_ctx_destroy(self.h)
            self.h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def load_index_files(self, prefix):
        _chk(lib().ibwa_ctx_load_bwt_file(self.h, 0, (prefix + ".bwt").encode()))
        _chk(lib().ibwa_ctx_load_bwt_file(self.h, 1, (prefix + ".rbwt").encode()))

    def load_index(self, strand, primary, L2, words):
        words = np.ascontiguousarray(words, dtype=np.uint32)
        arr = (c.c_uint32 * 4)(*[int(x) for x in L2])
        _chk(lib().ibwa_ctx_load_bwt(self.h, strand, int(primary), arr, words.ctypes.data, words.size))

    def share_index(self, src):
        """Borrow src's resident index (ibwa_ctx_share_index); src must outlive this engine."""
        _chk(lib().ibwa_ctx_share_index(self.h, src.h))
        self._share_src = src

    def set_tuning(self, stack_cap=0, aln_cap=0, block=0):
        _chk(lib().ibwa_ctx_set_tuning(self.h, stack_cap, aln_cap, block))

    def set_option(self, key, value):
        _chk(lib().ibwa_ctx_set_option(self.h, key.encode(), int(value)))

    def stage(self, seqs, offs, lens):
        self._keep = (np.ascontiguousarray(seqs, dtype=np.uint8), np.ascontiguousarray(offs, dtype=np.uint64),
                      np.ascontiguousarray(lens, dtype=np.uint32))
        s, o, l = self._keep
        _chk(lib().ibwa_batch_stage(self.h, l.size, s.ctypes.data, o.ctypes.data, l.ctypes.data))
        self.n = l.size

    def fq_parse(self, raw, barcode=0, trim_qual=0, il13=False, cap=None):
        """ibwa_fq_parse over one raw block (bytes, or a uint8 array -- e.g. a view of ibwa_host_alloc memory):
        (n_rec, consumed, not_strict, rec_len int32[n_rec], rec_L uint32[n_rec]).  cap=None: the CLI's
        len(raw) // 48 + 17 (ingest.h).  The kept reads stay in the context (fq_kept, stage_fq)."""
        if isinstance(raw, np.ndarray):
            a = np.ascontiguousarray(raw, dtype=np.uint8)
        else:
            a = np.frombuffer(bytes(raw) or b"\0", dtype=np.uint8)
        nbytes = len(raw)
        if cap is None:
            cap = nbytes // 48 + 17
        n_rec, consumed, not_strict = c.c_int64(), c.c_uint64(), c.c_int()
        rec_len = np.zeros(max(cap, 1), np.int32)
        rec_L = np.zeros(max(cap, 1), np.uint32)
        mode = (int(barcode) << 24) | (MODE_IL13 if il13 else 0)
        _chk(lib().ibwa_fq_parse(self.h, a.ctypes.data, nbytes, mode, int(trim_qual), c.byref(n_rec), c.byref(consumed),
                                 c.byref(not_strict), rec_len.ctypes.data, rec_L.ctypes.data, cap))
        self._fq_nbytes = nbytes
        n = n_rec.value
        return n, consumed.value, not_strict.value, rec_len[:n].copy(), rec_L[:n].copy()

    def fq_stats(self):
        """(kept reads, device ms) of the last fq_parse (ibwa_fq_stats)."""
        kept, ms = c.c_int64(), c.c_double()
        _chk(lib().ibwa_fq_stats(self.h, c.byref(kept), c.byref(ms)))
        return kept.value, ms.value

    def fq_offset(self, r):
        """Byte offset of record r in the last parsed block (ibwa_fq_offset)."""
        off = c.c_uint64()
        _chk(lib().ibwa_fq_offset(self.h, int(r), c.byref(off)))
        return off.value

    def fq_kept(self, first=0, n=None):
        """Kept reads [first, first + n) of the last parsed block as the device holds them (ibwa_fq_fetch):
        (codes uint8 -- the bytes the reads span, off uint64[n] -- absolute, lens uint32[n]).  n=None: to the last."""
        if n is None:
            n = self.fq_stats()[0] - first
        lens = np.zeros(max(n, 1), np.uint32)
        off = np.zeros(max(n, 1), np.uint64)
        codes = np.zeros(getattr(self, "_fq_nbytes", 0) // 2 + 16, np.uint8)
        _chk(lib().ibwa_fq_fetch(self.h, int(first), int(n), lens.ctypes.data, off.ctypes.data, codes.ctypes.data,
                                 codes.size))
        n = max(n, 0)
        lens, off = lens[:n], off[:n]
        nb = int(off[-1] + lens[-1] - off[0]) if n else 0
        return codes[:nb].copy(), off.copy(), lens.copy()

    def stage_fq(self, src, first, n, max_len):
        """Stage kept reads [first, first + n) of src's last parsed block as this context's batch
        (ibwa_batch_stage_fq: a view, nothing is copied)."""
        _chk(lib().ibwa_batch_stage_fq(self.h, src.h, int(first), int(n), int(max_len)))
        self.n = int(n)

    def run(self, opt, batch_max_len=0):
        _chk(lib().ibwa_batch_run(self.h, c.byref(opt), batch_max_len))

    def fetch(self):
        n_aln = np.zeros(self.n, dtype=np.int32)
        ptr = c.c_void_p()
        tot = c.c_int64()
        _chk(lib().ibwa_batch_fetch(self.h, n_aln.ctypes.data, c.byref(ptr), c.byref(tot)))
        buf = c.string_at(ptr.value, tot.value * 16)
        lib().ibwa_free(ptr)
        return n_aln, np.frombuffer(buf, dtype=ALN_DTYPE).copy()

    def fetch_sai(self):
        """The batch's .sai records (ibwa_batch_fetch_sai): per read int32 n_aln + n_aln records."""
        need = c.c_uint64()
        _chk(lib().ibwa_batch_fetch_sai(self.h, None, 0, c.byref(need), None))
        buf = c.create_string_buffer(max(need.value, 1))
        _chk(lib().ibwa_batch_fetch_sai(self.h, buf, need.value, c.byref(need), None))
        return buf.raw[:need.value]

    def retry_info(self):
        """(read ids, pass) of the reads the last run's first pass handed on; pass 1 = coop,
        2 = sequential wide, 3 = general kernels, 4 = coop resuming the first pass's state."""
        n = c.c_int64()
        _chk(lib().ibwa_batch_retry_info(self.h, None, None, 0, c.byref(n)))
        ids = np.zeros(n.value, np.int64)
        ps = np.zeros(n.value, np.uint8)
        _chk(lib().ibwa_batch_retry_info(self.h, ids.ctypes.data, ps.ctypes.data, n.value, c.byref(n)))
        return ids, ps

    def diag(self):
        """(first-pass iterations uint32[n], k_width features uint16[n, 4]) of the last run (option diag=1)."""
        it = np.zeros(self.n, np.uint32)
        ft = np.zeros((self.n, 4), np.uint16)
        _chk(lib().ibwa_batch_diag(self.h, 0, it.ctypes.data, it.nbytes))
        _chk(lib().ibwa_batch_diag(self.h, 1, ft.ctypes.data, ft.nbytes))
        return it, ft

    def handoff_pops(self):
        """Per read: pops the first pass made before leaving its resume state (0: none), ibwa_batch_diag 2."""
        hp = np.zeros(self.n, np.uint32)
        _chk(lib().ibwa_batch_diag(self.h, 2, hp.ctypes.data, hp.nbytes))
        return hp

    def _width_shape(self):
        sh = np.zeros(3, np.uint64)
        _chk(lib().ibwa_batch_diag(self.h, 5, sh.ctypes.data, sh.nbytes))
        return int(sh[0]), int(sh[1]), int(sh[2])

    def width_rows(self):
        """The first-pass chunk's width rows as k_width wrote them, uint32[reads, wstride, 2] of {width, bid}
        (option diag_width=1, a batch of one chunk), ibwa_batch_diag 3."""
        n, ws, _ = self._width_shape()
        w = np.zeros((n, ws, 2), np.uint32)
        _chk(lib().ibwa_batch_diag(self.h, 3, w.ctypes.data, w.nbytes))
        return w

    def width_records(self):
        """Its compact records, uint32[reads, cw_words]; no rows when the first pass ran without them
        (option diag_width=1), ibwa_batch_diag 4."""
        n, _, cw = self._width_shape()
        r = np.zeros((n if cw else 0, cw), np.uint32)
        _chk(lib().ibwa_batch_diag(self.h, 4, r.ctypes.data, r.nbytes))
        return r

    @staticmethod
    def device_bytes():
        """(bytes held now, high-water mark) of the library's device buffers, all contexts of the process."""
        now, peak = c.c_int64(), c.c_int64()
        _chk(lib().ibwa_device_bytes(c.byref(now), c.byref(peak)))
        return now.value, peak.value

    def stats(self):
        st = RunStats()
        _chk(lib().ibwa_batch_stats(self.h, c.byref(st)))
        return st

    def aln(self, seqs, offs, lens, opt, batch_max_len=0):
        """bwa_cal_sa_reg_gap over one batch -> (n_aln[n], alns ALN_DTYPE)."""
        self.stage(seqs, offs, lens)
        self.run(opt, batch_max_len)
        return self.fetch()

    def build_index(self, codes, sa_intv=0):
        """On-device `bwa index` (BWT part) from 2-bit codes (uint8, N already replaced)."""
        codes = np.ascontiguousarray(codes, dtype=np.uint8)
        _chk(lib().ibwa_ctx_build_index(self.h, codes.ctypes.data, codes.size, sa_intv))

    def bwt_info(self, strand):
        p = c.c_uint32()
        L2 = (c.c_uint32 * 4)()
        sz = c.c_uint64()
        _chk(lib().ibwa_ctx_bwt_info(self.h, strand, c.byref(p), L2, c.byref(sz)))
        return p.value, tuple(L2), sz.value

    def export_bwt(self, strand):
        """-> (primary, L2[1..4], words) in the reference .bwt layout."""
        primary, L2, sz = self.bwt_info(strand)
        words = np.zeros(sz, dtype=np.uint32)
        _chk(lib().ibwa_ctx_export_bwt(self.h, strand, words.ctypes.data, sz))
        return primary, L2, words

    def export_sa(self, strand, intv):
        n = self.bwt_info(strand)[1][3]
        out = np.zeros((n + intv) // intv, dtype=np.uint32)
        _chk(lib().ibwa_ctx_export_sa(self.h, strand, out.ctypes.data, out.size))
        return out

    def build_rounds(self, strand):
        """Sort rounds build_index took for this strand (prefix doubling from 21 symbols)."""
        r = c.c_int()
        _chk(lib().ibwa_ctx_build_rounds(self.h, strand, c.byref(r)))
        return r.value

    def load_sa_files(self, prefix):
        """bwt_restore_sa (bwtio.c:29) of prefix.sa / prefix.rsa onto the device."""
        _chk(lib().ibwa_ctx_load_sa_file(self.h, 0, (prefix + ".sa").encode()))
        _chk(lib().ibwa_ctx_load_sa_file(self.h, 1, (prefix + ".rsa").encode()))

    def load_sa(self, strand, sa, intv):
        sa = np.ascontiguousarray(sa, dtype=np.uint32)
        _chk(lib().ibwa_ctx_load_sa(self.h, strand, int(intv), sa.ctypes.data, sa.size))

    def derive_sa(self, intv=32):
        """Sampled SA of both strands derived on the device from the resident BWT alone."""
        _chk(lib().ibwa_ctx_derive_sa(self.h, intv))

    def expand_sa(self):
        _chk(lib().ibwa_ctx_expand_sa(self.h))

    def prepare(self, opt):
        """The per-index device structures the first run with `opt` needs (ibwa_ctx_prepare)."""
        _chk(lib().ibwa_ctx_prepare(self.h, c.byref(opt)))

    def sa2pos(self, strand, k, lens, offset=0):
        """bwtdb_sa2seq (dbset.c:240-246) for arrays of hits -> uint64 positions."""
        strand = np.ascontiguousarray(strand, dtype=np.uint8)
        k = np.ascontiguousarray(k, dtype=np.uint32)
        lens = np.ascontiguousarray(lens, dtype=np.uint32)
        pos = np.zeros(k.size, dtype=np.uint64)
        _chk(lib().ibwa_sa2pos(self.h, k.size, strand.ctypes.data, k.ctypes.data, lens.ctypes.data, int(offset),
                               pos.ctypes.data))
        return pos

    def paired_sw(self, seqs0, seqs1, pe_opt, ii, pac, l_pac):
        """bwa_paired_sw (bwasw.c:270) over two RefSeq arrays (mutated in place);
        pac = the packed .pac bytes.  Returns [mated singletons, singletons, fixed, discordant]."""
        arr = (c.POINTER(RefSeq) * 2)(c.cast(seqs0, c.POINTER(RefSeq)), c.cast(seqs1, c.POINTER(RefSeq)))
        pac = np.ascontiguousarray(pac, dtype=np.uint8)
        tot = (c.c_uint64 * 2)()
        mapped = (c.c_uint64 * 2)()
        _chk(lib().ibwa_paired_sw(self.h, len(seqs0), arr, c.byref(pe_opt), c.byref(ii), pac.ctypes.data, int(l_pac),
                                  tot, mapped))
        return [mapped[1], tot[1], mapped[0], tot[0]]

    def global_align(self, refs, reads, band=50, gap_end=5):
        """Batched aln_global_core (stdaln.c:345) with aln_param_bwa scores -> list of
        (score, path_len, cigar str) per pair."""
        n = len(refs)
        o1 = np.zeros(n, np.uint64)
        o2 = np.zeros(n, np.uint64)
        l1 = np.array([len(x) for x in refs], np.uint32)
        l2 = np.array([len(x) for x in reads], np.uint32)
        if n:
            o1[1:] = np.cumsum(l1[:-1])
            o2[1:] = np.cumsum(l2[:-1])
        s1 = np.concatenate([np.asarray(x, np.uint8) for x in refs] + [np.zeros(1, np.uint8)])
        s2 = np.concatenate([np.asarray(x, np.uint8) for x in reads] + [np.zeros(1, np.uint8)])
        score = np.zeros(n, np.int32)
        plen = np.zeros(n, np.int32)
        ncig = np.zeros(n, np.int32)
        ptr = c.c_void_p()
        tot = c.c_int64()
        _chk(lib().ibwa_global_batch(self.h, n, s1.ctypes.data, o1.ctypes.data, l1.ctypes.data, s2.ctypes.data,
                                     o2.ctypes.data, l2.ctypes.data, band, gap_end, score.ctypes.data,
                                     plen.ctypes.data, ncig.ctypes.data, c.byref(ptr), c.byref(tot)))
        cig = np.frombuffer(c.string_at(ptr.value, 4 * max(tot.value, 0)), dtype=np.uint32).copy()
        lib().ibwa_free(ptr)
        out, q = [], 0
        for p in range(n):
            out.append((int(score[p]), int(plen[p]),
                        "".join(f"{x >> 4}{'MIDS'[x & 0xf]}" for x in cig[q:q + ncig[p]])))
            q += ncig[p]
        return out

    def stdaln(self, seq1s, seq2s, param, mode="local", thres=1):
        """Batched aln_local_core / aln_global_core / aln_extend_core (mode "local", "global", "extend": the
        last is aln_stdaln_aux's type 2, G0 = 1 with the path) for any scoring scheme (ibwa_stdaln_batch).
        seq1s / seq2s: code arrays (each code < row); param: a preset name, aln_param()'s dict, or a
        (gap_open, gap_ext, gap_end, matrix, row, band_width) tuple (band_width <= 0: len1 + len2).
        Returns per pair (score, subo, path_len, start (i, j) | None, end (i, j) | None, cigar str |
        None); as in aln_stdaln_aux a start coordinate of 0 is given as 1."""
        ap, _mat = _aln_param_struct(param)
        n, s1, o1, l1, s2, o2, l2 = _pair_arrays(seq1s, seq2s)
        score = np.zeros(n, np.int32)
        subo = np.zeros(n, np.int32)
        plen = np.zeros(n, np.int32)
        ends = np.zeros((n, 4), np.int32)
        ncig = np.zeros(n, np.int32)
        ptr = c.c_void_p()
        tot = c.c_int64()
        _chk(lib().ibwa_stdaln_batch(self.h, c.byref(ap), _STDALN_TYPES[mode], thres, n, s1.ctypes.data,
                                     o1.ctypes.data, l1.ctypes.data, s2.ctypes.data, o2.ctypes.data, l2.ctypes.data,
                                     score.ctypes.data, subo.ctypes.data, plen.ctypes.data, ends.ctypes.data,
                                     ncig.ctypes.data, c.byref(ptr), c.byref(tot)))
        cig = np.frombuffer(c.string_at(ptr.value, 4 * max(tot.value, 0)), dtype=np.uint32).copy()
        lib().ibwa_free(ptr)
        out, q = [], 0
        for p in range(n):
            if plen[p] > 0:
                cs = "".join(f"{x >> 4}{'MIDS'[x & 0xf]}" for x in cig[q:q + ncig[p]])
                out.append((int(score[p]), int(subo[p]), int(plen[p]), (int(ends[p, 0]) or 1, int(ends[p, 1]) or 1),
                            (int(ends[p, 2]), int(ends[p, 3])), cs))
            else:
                out.append((int(score[p]), int(subo[p]), 0, None, None, None))
            q += ncig[p]
        return out

    def stdaln_chunks(self):
        """(launches, kernel ms) of the last stdaln call."""
        k, ms = c.c_int64(), c.c_double()
        _chk(lib().ibwa_stdaln_chunks(self.h, c.byref(k), c.byref(ms)))
        return k.value, ms.value

    def extend(self, seq1s, seq2s, param, g0=1, mode="end"):
        """Batched aln_extend_core (ibwa_extend_batch).  g0: one value or one per pair.  Returns per pair
        (score, end (i, j) | None) in mode "end", (score, None) in mode "score", and (score, end | None,
        path_len, cigar str | None) in mode "path" (score: the global fill's, as the reference returns it)."""
        ap, _mat = _aln_param_struct(param)
        n, s1, o1, l1, s2, o2, l2 = _pair_arrays(seq1s, seq2s)
        g = _g0_array(g0, n)
        m = _EXTEND_MODES[mode]
        score = np.zeros(n, np.int32)
        ends = np.zeros((n, 2), np.int32)
        plen = np.zeros(n, np.int32)
        ncig = np.zeros(n, np.int32)
        ptr = c.c_void_p()
        tot = c.c_int64()
        _chk(lib().ibwa_extend_batch(self.h, c.byref(ap), m, n, s1.ctypes.data, o1.ctypes.data, l1.ctypes.data,
                                     s2.ctypes.data, o2.ctypes.data, l2.ctypes.data, None if g is None else g.ctypes.data,
                                     score.ctypes.data, ends.ctypes.data, plen.ctypes.data, ncig.ctypes.data,
                                     c.byref(ptr), c.byref(tot)))
        cig = np.zeros(0, np.uint32)
        if ptr.value:
            cig = np.frombuffer(c.string_at(ptr.value, 4 * max(tot.value, 0)), dtype=np.uint32).copy()
            lib().ibwa_free(ptr)
        out, q = [], 0
        for p in range(n):
            has_end = score[p] > 0 if m == 1 else plen[p] > 0  # path mode: the global score may be <= 0 beside a path
            end = (int(ends[p, 0]), int(ends[p, 1])) if has_end else None
            if m < 2:
                out.append((int(score[p]), end))
            elif plen[p] > 0:
                out.append((int(score[p]), end, int(plen[p]),
                            "".join(f"{x >> 4}{'MIDS'[x & 0xf]}" for x in cig[q:q + ncig[p]])))
            else:
                out.append((int(score[p]), None, 0, None))
            q += ncig[p]
        return out

    def extend_seeds(self, pos, dirs, lts, queries, param, g0=1, rev=False):
        """End-cell extension of seeds against the resident sequence (ibwa_extend_seeds): seed p reads at most
        lts[p] bases rightwards from pos[p] (dirs[p] == 0) or leftwards from pos[p] - 1 (dirs[p] == 1);
        queries[p]: the codes in the order the DP consumes them.  Returns per seed (score, end (i, j) | None)."""
        pos = np.ascontiguousarray(pos, dtype=np.uint64)
        dirs = np.ascontiguousarray(dirs, dtype=np.uint8)
        lts = np.ascontiguousarray(lts, dtype=np.uint32)
        n = len(queries)
        if not (pos.size == dirs.size == lts.size == n):
            raise IbwaError("extend_seeds: pos, dirs, lts and queries differ in length")
        ap, _mat = _aln_param_struct(param)
        s, off, ln = self._pack_reads(queries)
        g = _g0_array(g0, n)
        score = np.zeros(n, np.int32)
        ends = np.zeros((n, 2), np.int32)
        _chk(lib().ibwa_extend_seeds(self.h, c.byref(ap), n, pos.ctypes.data, dirs.ctypes.data, lts.ctypes.data, int(bool(rev)),
                                     s.ctypes.data, off.ctypes.data, ln.ctypes.data, None if g is None else g.ctypes.data,
                                     score.ctypes.data, ends.ctypes.data))
        return [(int(score[p]), (int(ends[p, 0]), int(ends[p, 1])) if score[p] > 0 else None) for p in range(n)]

    def bwasw_seeds(self, seqs, strands, opt="bwasw", adjust=True):
        """bwasw's seeding (ibwa_bsw2_seed_batch): bsw2_core of every task -- seqs[i], codes 0-3, against
        .bwt / .sa (strands[i] == 0) or .rbwt / .rsa (1).  opt: see bsw2_opt; adjust: t and bw follow each
        read's length as in bsw2_aln_core.  Returns per task (all_hits, narrow_hits), lists of
        (k, l, flag, len, G, G2, beg, end) tuples in the reference's order after bsw2_resolve_duphits."""
        o = bsw2_opt(opt, adjust)
        s, off, ln = self._pack_reads(seqs)
        st = np.ascontiguousarray(strands, dtype=np.uint8)
        n = ln.size
        if st.size != n:
            raise IbwaError("bsw2 seed: seqs and strands differ in length")
        n_all = np.zeros(n, np.int32)
        n_nar = np.zeros(n, np.int32)
        ptr = c.c_void_p()
        tot = c.c_int64()
        _chk(lib().ibwa_bsw2_seed_batch(self.h, c.byref(o), n, s.ctypes.data, off.ctypes.data, ln.ctypes.data,
                                        st.ctypes.data, n_all.ctypes.data, n_nar.ctypes.data, c.byref(ptr), c.byref(tot)))
        try:
            buf = (c.c_char * (tot.value * BSW2_HIT_DTYPE.itemsize)).from_address(ptr.value) if tot.value else b""
            hits = [tuple(int(x) for x in h) for h in np.frombuffer(buf, dtype=BSW2_HIT_DTYPE).tolist()]
        finally:
            lib().ibwa_free(ptr)
        out, at = [], 0
        for i in range(n):
            a, b = int(n_all[i]), int(n_nar[i])
            out.append((hits[at:at + a], hits[at + a:at + a + b]))
            at += a + b
        return out

    def bwasw_hits(self, seqs, is_rev, opt="bwasw", adjust=True, u=None):
        """bwasw from reads to hits on one index strand (ibwa_bsw2_aln1_batch): bsw2_aln1_core of every read
        -- seqs[i], codes 0-3, against .bwt / .sa with the target read forwards (is_rev[i] == 0), or the
        reversed read against .rbwt / .rsa with the target read through __rpac (1).  opt: see bsw2_aln_opt;
        u: per read the draw of bsw2_resolve_query_overlaps in [0, 1) (None: 0.0).  Returns per read the
        list of (k, l, flag, n_seeds, len, G, G2, beg, end) tuples in the reference's order."""
        o = bsw2_aln_opt(opt, adjust)
        s, off, ln = self._pack_reads(seqs)
        rv = np.ascontiguousarray(is_rev, dtype=np.uint8)
        uu = None if u is None else np.ascontiguousarray(u, dtype=np.float64)
        n = ln.size
        if rv.size != n or (uu is not None and uu.size != n):
            raise IbwaError("bsw2 aln1: seqs, is_rev and u differ in length")
        cnt = np.zeros(n, np.int32)
        ptr = c.c_void_p()
        tot = c.c_int64()
        _chk(lib().ibwa_bsw2_aln1_batch(self.h, c.byref(o), n, s.ctypes.data, off.ctypes.data, ln.ctypes.data, rv.ctypes.data,
                                        None if uu is None else uu.ctypes.data, cnt.ctypes.data, c.byref(ptr), c.byref(tot)))
        try:
            buf = (c.c_char * (tot.value * BSW2_ALN_HIT_DTYPE.itemsize)).from_address(ptr.value) if tot.value else b""
            hits = [tuple(int(x) for x in h) for h in np.frombuffer(buf, dtype=BSW2_ALN_HIT_DTYPE).tolist()]
        finally:
            lib().ibwa_free(ptr)
        out, at = [], 0
        for i in range(n):
            out.append(hits[at:at + int(cnt[i])])
            at += int(cnt[i])
        return out

    def bwasw_extend_left(self, queries, bws, is_rev, hit_lists, opt="bwasw"):
        """bsw2_extend_left alone (ibwa_bsw2_extend_left_batch): per task a query (the strand's sequence, codes
        0-3), a band, is_rev and a list of (k, l, flag, n_seeds, len, G, G2, beg, end) in any order.  Returns
        per task the list sorted by end, descending, with G, len, beg, k and n_seeds as the reference leaves
        them.  Of opt only a, b, q, r are read."""
        o = bsw2_opt(opt)
        s, off, ln = self._pack_reads(queries)
        n = ln.size
        bw = np.ascontiguousarray(bws, dtype=np.int32)
        rv = np.ascontiguousarray(is_rev, dtype=np.uint8)
        if bw.size != n or rv.size != n or len(hit_lists) != n:
            raise IbwaError("bsw2 extend_left: queries, bws, is_rev and hit_lists differ in length")
        cnt = np.array([len(h) for h in hit_lists], np.int32)
        flat = [tuple(h) for hs in hit_lists for h in hs]
        hits = np.array(flat, dtype=BSW2_ALN_HIT_DTYPE) if flat else np.zeros(1, BSW2_ALN_HIT_DTYPE)
        _chk(lib().ibwa_bsw2_extend_left_batch(self.h, c.byref(o), n, s.ctypes.data, off.ctypes.data, ln.ctypes.data,
                                               bw.ctypes.data, rv.ctypes.data, cnt.ctypes.data, hits.ctypes.data))
        rows = [tuple(int(x) for x in h) for h in hits.tolist()] if flat else []
        out, at = [], 0
        for i in range(n):
            out.append(rows[at:at + int(cnt[i])])
            at += int(cnt[i])
        return out

    def bwasw_hits_stats(self):
        """The last bwasw_hits or bwasw_extend_left call: microseconds of the left and the right launch; of
        the left launch the hits extended (DP runs that counted), those skipped as contained before any
        DP, the speculative DP runs discarded, the hits skipped for l != 0 or k == 0, its tasks and its
        windows of 64."""
        v = (c.c_int64 * 8)()
        _chk(lib().ibwa_bsw2_aln1_stats(self.h, c.byref(v)))
        return dict(zip(("us_left", "us_right", "extended", "contained", "discarded", "skipped", "tasks", "windows"),
                        [int(x) for x in v]))

    def seed_stats(self):
        """The last bwasw_seeds call: wall-clock ticks its waves spent in bwtl build, traversal and resolve,
        cells visited, tasks run again, the largest arena a task used and the first launch's arena (bytes),
        and its workgroups."""
        v = (c.c_int64 * 8)()
        _chk(lib().ibwa_bsw2_seed_stats(self.h, c.byref(v)))
        return dict(zip(("ticks_build", "ticks_walk", "ticks_resolve", "cells", "retried", "arena_peak", "arena",
                         "workgroups"), [int(x) for x in v]))

    def extend_stats(self):
        """{"no_band": path-mode pairs of the last extension whose global fill stayed below the extension
        score (the reference's 'no suitable bandwidth' line)}."""
        k = c.c_int64()
        _chk(lib().ibwa_extend_stats(self.h, c.byref(k)))
        return {"no_band": k.value}

    def sw(self, refs, reads):
        """Batched aln_local_core (stdaln.c:529) over code arrays.  Returns a list of
        (score, path_len, start (i, j) | None, end (i, j) | None, cigar str | None)."""
        n = len(refs)
        o1 = np.zeros(n, np.uint64)
        o2 = np.zeros(n, np.uint64)
        l1 = np.array([len(x) for x in refs], np.uint32)
        l2 = np.array([len(x) for x in reads], np.uint32)
        if n:
            o1[1:] = np.cumsum(l1[:-1])
            o2[1:] = np.cumsum(l2[:-1])
        s1 = np.concatenate([np.asarray(x, np.uint8) for x in refs] + [np.zeros(1, np.uint8)])
        s2 = np.concatenate([np.asarray(x, np.uint8) for x in reads] + [np.zeros(1, np.uint8)])
        score = np.zeros(n, np.int32)
        plen = np.zeros(n, np.int32)
        ends = np.zeros((n, 4), np.int32)
        ncig = np.zeros(n, np.int32)
        ptr = c.c_void_p()
        tot = c.c_int64()
        _chk(lib().ibwa_sw_batch(self.h, n, s1.ctypes.data, o1.ctypes.data, l1.ctypes.data, s2.ctypes.data,
                                 o2.ctypes.data, l2.ctypes.data, score.ctypes.data, plen.ctypes.data,
                                 ends.ctypes.data, ncig.ctypes.data, c.byref(ptr), c.byref(tot)))
        cig = np.frombuffer(c.string_at(ptr.value, 4 * max(tot.value, 0)), dtype=np.uint32).copy()
        lib().ibwa_free(ptr)
        out, q = [], 0
        for p in range(n):
            if score[p] >= 0 and plen[p] > 0:
                cs = "".join(f"{x >> 4}{'MIDS'[x & 0xf]}" for x in cig[q:q + ncig[p]])
                out.append((int(score[p]), int(plen[p]), (int(ends[p, 0]), int(ends[p, 1])),
                            (int(ends[p, 2]), int(ends[p, 3])), cs))
            else:
                out.append((int(score[p]), int(plen[p]), None, None, None))
            q += ncig[p]
        return out

    def sw_core(self, reads, windows, reglen, beg, l_pac):
        """bwa_sw_core (bwasw.c:29-112) per mate rescue, batched.  Returns a list of
        None (rejected) or (beg, [bwa_cigar_t ...], cnt)."""
        n = len(reads)
        off = np.zeros(n, np.uint64)
        roff = np.zeros(n, np.uint64)
        ln = np.array([len(x) for x in reads], np.uint32)
        rl = np.array([len(x) for x in windows], np.uint32)
        if n:
            off[1:] = np.cumsum(ln[:-1])
            roff[1:] = np.cumsum(rl[:-1])
        s = np.concatenate([np.asarray(x, np.uint8) for x in reads] + [np.zeros(1, np.uint8)])
        r = np.concatenate([np.asarray(x, np.uint8) for x in windows] + [np.zeros(1, np.uint8)])
        rg = np.ascontiguousarray(reglen, np.int32)
        bg = np.ascontiguousarray(beg, np.int64).copy()
        nc = np.zeros(n, np.int32)
        cnt = np.zeros(n, np.uint32)
        ptr = c.c_void_p()
        _chk(lib().ibwa_sw_core_batch(self.h, n, s.ctypes.data, off.ctypes.data, ln.ctypes.data, r.ctypes.data,
                                      roff.ctypes.data, rl.ctypes.data, rg.ctypes.data, bg.ctypes.data, int(l_pac),
                                      nc.ctypes.data, cnt.ctypes.data, c.byref(ptr)))
        tot = int(nc.sum())
        cig = np.frombuffer(c.string_at(ptr.value, 4 * tot), dtype=np.uint32).copy() if tot else np.zeros(0, np.uint32)
        lib().ibwa_free(ptr)
        out, q = [], 0
        for p in range(n):
            if nc[p]:
                out.append((int(bg[p]), [int(x) for x in cig[q:q + nc[p]]], int(cnt[p])))
            else:
                out.append(None)
            q += nc[p]
        return out

    def load_pac(self, pacs, l_pacs):
        """The set's references (their .pac bytes and l_pac) back to back onto the device (ibwa_ctx_load_pac)."""
        keep = [np.ascontiguousarray(np.frombuffer(bytes(p), np.uint8) if not isinstance(p, np.ndarray) else p,
                                     dtype=np.uint8) for p in pacs]
        ptrs = (c.c_void_p * len(keep))(*[k.ctypes.data for k in keep])
        ls = (c.c_uint64 * len(keep))(*[int(x) for x in l_pacs])
        _chk(lib().ibwa_ctx_load_pac(self.h, len(keep), ptrs, ls))

    def pac_extract(self, beg, lens):
        """dbset_extract_sequence per window -> (list of uint8 code arrays of got[i] bases, got)."""
        beg = np.ascontiguousarray(beg, dtype=np.uint64)
        lens = np.ascontiguousarray(lens, dtype=np.uint32)
        n = beg.size
        off = np.zeros(n, np.uint64)
        if n:
            off[1:] = np.cumsum(lens[:-1], dtype=np.uint64)
        out = np.full(int(lens.sum()) + 1, 0xFF, np.uint8)
        got = np.zeros(n, np.uint32)
        _chk(lib().ibwa_pac_extract(self.h, n, beg.ctypes.data, lens.ctypes.data, off.ctypes.data, out.ctypes.data,
                                    got.ctypes.data))
        return [out[int(off[i]):int(off[i]) + int(got[i])].copy() for i in range(n)], got

    @staticmethod
    def _pack_reads(reads):
        n = len(reads)
        ln = np.array([len(x) for x in reads], np.uint32)
        off = np.zeros(n, np.uint64)
        if n:
            off[1:] = np.cumsum(ln[:-1], dtype=np.uint64)
        s = np.concatenate([np.asarray(x, np.uint8) for x in reads] + [np.zeros(1, np.uint8)])
        return s, off, ln

    def refine(self, pos, ext, reads, pos_out=None, n_cigar=None):
        """refine_gapped_core per job (ibwa_refine_batch) -> (pos' uint64[n], list of bwa_cigar_t arrays).
        pos_out / n_cigar: the output arrays to use (tests: a failed call leaves them untouched)."""
        n = len(reads)
        pos = np.ascontiguousarray(pos, dtype=np.uint64)
        ext = np.ascontiguousarray(ext, dtype=np.int32)
        s, off, ln = self._pack_reads(reads)
        po = np.zeros(n, np.uint64) if pos_out is None else pos_out
        nc = np.zeros(n, np.int32) if n_cigar is None else n_cigar
        ptr = c.c_void_p()
        tot = c.c_int64()
        _chk(lib().ibwa_refine_batch(self.h, n, pos.ctypes.data, ext.ctypes.data, s.ctypes.data, off.ctypes.data,
                                     ln.ctypes.data, po.ctypes.data, nc.ctypes.data, c.byref(ptr), c.byref(tot)))
        cig = np.frombuffer(c.string_at(ptr.value, 4 * max(tot.value, 0)), dtype=np.uint32).copy()
        lib().ibwa_free(ptr)
        assert tot.value == int(nc.sum())
        ends = np.concatenate([[0], np.cumsum(nc)])
        return po, [cig[ends[i]:ends[i + 1]] for i in range(n)]

    def md(self, pos, reads, cigars=None, raw=False):
        """bwa_cal_md1 per read (ibwa_md_batch); cigars: None, or per read None / a bwa_cigar_t sequence.
        -> (list of MD strings, nm int32[n]); raw=True: (offsets uint64[n + 1], text bytes, nm)."""
        n = len(reads)
        pos = np.ascontiguousarray(pos, dtype=np.uint64)
        s, off, ln = self._pack_reads(reads)
        nc = cg = None
        if cigars is not None:
            nc = np.array([-1 if x is None else len(x) for x in cigars], np.int32)
            cg = np.concatenate([np.asarray(x, np.uint32) for x in cigars if x is not None] + [np.zeros(1, np.uint32)])
        nm = np.zeros(n, np.int32)
        p_off, p_md = c.c_void_p(), c.c_void_p()
        _chk(lib().ibwa_md_batch(self.h, n, pos.ctypes.data, s.ctypes.data, off.ctypes.data, ln.ctypes.data,
                                 nc.ctypes.data if nc is not None else None, cg.ctypes.data if cg is not None else None,
                                 nm.ctypes.data, c.byref(p_off), c.byref(p_md)))
        offs = np.frombuffer(c.string_at(p_off.value, 8 * (n + 1)), dtype=np.uint64).copy()
        assert p_md.value == p_off.value + 8 * (n + 1)
        text = c.string_at(p_md.value, int(offs[n]))
        lib().ibwa_free(p_off)
        if raw:
            return offs, text, nm
        return [text[int(offs[i]):int(offs[i + 1]) - 1].decode() for i in range(n)], nm

    def pac2cspac(self, nt_pac, l_pac):
        """bwa_pac2cspac_core (ibwa_pac2cspac): a nucleotide .pac's bytes -> the l_pac // 4 + 1 colour bytes."""
        src = np.zeros((int(l_pac) + 3) // 4, np.uint8)
        have = np.frombuffer(bytes(nt_pac), np.uint8)[:src.size]
        src[:have.size] = have
        out = np.zeros(int(l_pac) // 4 + 1, np.uint8)
        _chk(lib().ibwa_pac2cspac(self.h, src.ctypes.data, int(l_pac), out.ctypes.data))
        return out

    def load_ntpac(self, pacs, l_pacs):
        """The nucleotide sequences of a colour-space set (their .nt.pac bytes and l_pac) onto the device
        (ibwa_ctx_load_ntpac)."""
        keep = [np.ascontiguousarray(np.frombuffer(bytes(p), np.uint8) if not isinstance(p, np.ndarray) else p,
                                     dtype=np.uint8) for p in pacs]
        ptrs = (c.c_void_p * len(keep))(*[k.ctypes.data for k in keep])
        ls = (c.c_uint64 * len(keep))(*[int(x) for x in l_pacs])
        _chk(lib().ibwa_ctx_load_ntpac(self.h, len(keep), ptrs, ls))

    def cs2nt_rows(self, nt_refs, cs_reads):
        """cs2nt_DP + cs2nt_nt_qual per row pair (ibwa_cs2nt_rows): nt_refs[i] has len(cs_reads[i]) + 1 codes
        -> list of uint8 arrays of len(cs_reads[i]) - 1 bytes, base << 6 | qual."""
        n = len(cs_reads)
        size = np.array([len(x) for x in cs_reads], np.uint32)
        assert all(len(r) == int(s) + 1 for r, s in zip(nt_refs, size))
        off = np.zeros(n + 1, np.uint64)
        off[1:] = np.cumsum(size.astype(np.uint64) + 1)
        ref = np.zeros(int(off[n]) + 1, np.uint8)
        cs = np.zeros(int(off[n]) + 1, np.uint8)
        for i in range(n):
            o = int(off[i])
            ref[o:o + int(size[i]) + 1] = nt_refs[i]
            cs[o:o + int(size[i])] = cs_reads[i]
        out = np.full(int(off[n]) + 1, 0xFF, np.uint8)
        _chk(lib().ibwa_cs2nt_rows(self.h, n, ref.ctypes.data, cs.ctypes.data, off.ctypes.data, size.ctypes.data,
                                   out.ctypes.data, off.ctypes.data))
        return [out[int(off[i]):int(off[i]) + int(size[i]) - 1].copy() for i in range(n)]

    def cs2nt(self, pos, strand, seqs, quals, cigars=None):
        """bwa_cs2nt_core's rows from the resident nucleotide sequence, then the DP (ibwa_cs2nt_batch).
        seqs[i]: colour codes in the hit's orientation; quals[i]: the quality string as read (bytes);
        cigars: None, or per read None / a bwa_cigar_t sequence -> list of uint8 arrays, base << 6 | qual."""
        n = len(seqs)
        pos = np.ascontiguousarray(pos, dtype=np.uint64)
        strand = np.ascontiguousarray(strand, dtype=np.uint8)
        s, off, ln = self._pack_reads(seqs)
        q, _, lq = self._pack_reads([np.frombuffer(bytes(x), np.uint8) for x in quals])
        assert (ln == lq).all()
        nc = cg = None
        if cigars is not None:
            nc = np.array([0 if x is None else len(x) for x in cigars], np.int32)
            cg = np.concatenate([np.asarray(x, np.uint32) for x in cigars if x is not None] + [np.zeros(1, np.uint32)])
        out = np.full(s.size, 0xFF, np.uint8)
        new_len = np.zeros(n, np.uint32)
        _chk(lib().ibwa_cs2nt_batch(self.h, n, pos.ctypes.data, strand.ctypes.data, s.ctypes.data, q.ctypes.data,
                                    off.ctypes.data, ln.ctypes.data, nc.ctypes.data if nc is not None else None,
                                    cg.ctypes.data if cg is not None else None, out.ctypes.data, new_len.ctypes.data))
        return [out[int(off[i]):int(off[i]) + int(new_len[i])].copy() for i in range(n)]

    def occ4(self, strand, ks):
        ks = np.ascontiguousarray(ks, dtype=np.uint32)
        out = np.zeros((ks.size, 4), dtype=np.uint32)
        _chk(lib().ibwa_occ4(self.h, strand, ks.size, ks.ctypes.data, out.ctypes.data))
        return out
