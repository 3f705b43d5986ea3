"""ctypes binding of libgtx.so (include/gtx.h) -- the MI355X interval-overlap engine.

Host language note: the reference is C++, so the product's host side is C++ (csrc/); this
module only exposes the C ABI to Python for the parity tests and bench.py.  It never computes
counts itself and has no CPU path: if libgtx.so is missing or no HIP device is usable it raises.
"""
import ctypes
import os

import numpy as np

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.environ.get("GTX_LIB_PATH") or os.path.join(os.path.dirname(_HERE), "csrc", "libgtx.so")   # GTX_LIB_PATH: diagnostic builds (make trace)

READS_SORTED = 1
CHECK_SORTED = 2
ZERO_LENGTH_OK = 4
GAPS_FORMULA = 8
READS_UNSORTED = 16
JOIN_GAPS = 32
OFFSET_SKIP_REF_GAPS = 64
OFFSET_FROM_QUERY = 128
SIGNAL_PER_REF = 256
TEXT_SAM = 512            # gtx_*_add_text: the block is SAM alignments, not BED
TEXT_GFF = 2048           # gtx_*_add_text: the block is GFF / GTF features, not BED
SUBSET_INVERT = 1024      # gtx_subset_text: keep the lines without hits (-inv)
LINK_SUM = 1              # gtx_link: fold the values (at most one of the three)
LINK_MIN = 2
LINK_MAX = 4
LINK_TILE = 2048          # GTX_LINK_TILE: regions per block of link's scans
ADJACENT_TILE = 2048      # GTX_ADJACENT_TILE: regions per block of the neighbour passes
POINTS = {"1": 0, "2": 1, "5p": 2, "3p": 3}   # GTX_POINT_*: gdist's reference points
SCAN_KEEP_SLOTS = 8       # GTX_SCAN_KEEP_SLOTS: window vectors a context keeps in HBM
FILTER_TILE = 1024        # GTX_FILTER_TILE: windows per tile of the window filter's passes
PEAK_TILE = 1024          # GTX_PEAK_TILE: windows per tile of the peak candidate selection's passes
OFFSET_OPS = {"1": 1, "2": 2, "5p": 3, "3p": 4}
ANNOTATE_CENTER = 1
ANNOTATE_START = 2
REFS_KEEP_ZERO_LENGTH = 1
GROUP_ID_BYTES = 128

_lib = None


class GtxError(RuntimeError):
    pass


class CountInfo(ctypes.Structure):
    _fields_ = [("first_unsorted", ctypes.c_int64), ("n_no_class", ctypes.c_int64),
                ("n_degenerate", ctypes.c_int64), ("first_degenerate", ctypes.c_int64), ("n_unplaced", ctypes.c_int64)]

    def as_dict(self):
        return {k: int(getattr(self, k)) for k, _ in self._fields_}


class SignalInfo(ctypes.Structure):
    _fields_ = [("n_pairs", ctypes.c_int64), ("n_binned", ctypes.c_int64), ("n_dropped", ctypes.c_int64),
                ("weight_abs_sum", ctypes.c_int64), ("n_no_class", ctypes.c_int64), ("n_degenerate", ctypes.c_int64)]

    def as_dict(self):
        return {k: int(getattr(self, k)) for k, _ in self._fields_}


class LinkInfo(ctypes.Structure):
    _fields_ = [("n_groups", ctypes.c_int64), ("first_unsorted", ctypes.c_int64)]

    def as_dict(self):
        return {k: int(getattr(self, k)) for k, _ in self._fields_}


class AdjacentInfo(ctypes.Structure):
    _fields_ = [("first_unsorted", ctypes.c_int64), ("n_inclusions", ctypes.c_int64), ("n_overlaps", ctypes.c_int64)]

    def as_dict(self):
        return {k: int(getattr(self, k)) for k, _ in self._fields_}


class GapsInfo(ctypes.Structure):
    _fields_ = [("n_gaps", ctypes.c_int64), ("first_bad", ctypes.c_int64), ("bad_kind", ctypes.c_int32)]

    def as_dict(self):
        return {k: int(getattr(self, k)) for k, _ in self._fields_}


class TextRules(ctypes.Structure):
    """gtx_text_rules (include/gtx.h): how the device reads a block of BED text"""
    _fields_ = [("chrom_names", ctypes.POINTER(ctypes.c_char_p)), ("n_chrom", ctypes.c_int32),
                ("strand_aware", ctypes.c_int32), ("sorted_rules", ctypes.c_int32), ("sorted_by_strand", ctypes.c_int32),
                ("max_label_value", ctypes.c_int64),
                ("have_prev", ctypes.c_int32), ("prev_chrom", ctypes.c_char_p), ("prev_strand", ctypes.c_int32), ("prev_start", ctypes.c_int64)]

    @classmethod
    def make(cls, names, strand_aware=False, sorted_rules=False, sorted_by_strand=False, max_label_value=1):
        r = cls()
        r._names = (ctypes.c_char_p * len(names))(*[n.encode() for n in names])     # (kept alive with the object)
        r.chrom_names = r._names; r.n_chrom = len(names)
        r.strand_aware = int(strand_aware); r.sorted_rules = int(sorted_rules); r.sorted_by_strand = int(sorted_by_strand)
        r.max_label_value = int(max_label_value); r.have_prev = 0; r.prev_chrom = None; r.prev_strand = ord("+"); r.prev_start = 0
        return r


REWRITE_SHIFT, REWRITE_SHIFTP, REWRITE_POS, REWRITE_CENTER, REWRITE_FIX, REWRITE_BOUNDS = range(6)   # gtx_rewrite_op.kind
REWRITE_KINDS = {"shift": REWRITE_SHIFT, "shiftp": REWRITE_SHIFTP, "pos": REWRITE_POS, "center": REWRITE_CENTER, "fix": REWRITE_FIX, "bounds": REWRITE_BOUNDS}
REWRITE_POS_OPS = {"1": 0, "2": 1, "5p": 2, "3p": 3, "c": 4}                                          # gtx_rewrite_op.pos_op


class RewriteOp(ctypes.Structure):
    """gtx_rewrite_op (include/gtx.h): one operation of genomic_regions over columns 2 and 3"""
    _fields_ = [("kind", ctypes.c_int32), ("pos_op", ctypes.c_int32), ("a", ctypes.c_int64), ("b", ctypes.c_int64),
                ("chrom_names", ctypes.POINTER(ctypes.c_char_p)), ("chrom_len", ctypes.POINTER(ctypes.c_int64)), ("n_chrom", ctypes.c_int32)]

    @classmethod
    def make(cls, kind, a=0, b=0, pos_op="1", genome=None):
        """kind: a word of REWRITE_KINDS; genome: {name: length} for bounds"""
        o = cls()
        o.kind = REWRITE_KINDS[kind]; o.pos_op = REWRITE_POS_OPS[pos_op]; o.a = int(a); o.b = int(b)
        names = sorted(genome) if genome else []
        o._names = (ctypes.c_char_p * max(len(names), 1))(*[n.encode() for n in names])   # (kept alive with the object)
        o._lens = (ctypes.c_int64 * max(len(names), 1))(*[int(genome[n]) for n in names])
        o.chrom_names = o._names; o.chrom_len = o._lens; o.n_chrom = len(names)
        return o


class WindowsOp(ctypes.Structure):
    """gtx_windows_op (include/gtx.h): -s, -d and --small of genomic_regions win"""
    _fields_ = [("win_size", ctypes.c_int64), ("win_step", ctypes.c_int64), ("small", ctypes.c_int32)]

    @classmethod
    def make(cls, size=1, step=1, small=False):
        o = cls()
        o.win_size = int(size); o.win_step = int(step); o.small = int(bool(small))
        return o


BLOCKS_KINDS = {"split": 0, "connect": 1, "select": 2, "diff": 3, "n": 4, "strand": 5}                # gtx_blocks_op.kind
BLOCKS_FIRST, BLOCKS_LAST, BLOCKS_5P, BLOCKS_3P = 1, 2, 4, 8                                          # gtx_blocks_op.select
BLOCKS_STRAND_OPS = {"+": 0, "-": 1, "r": 2}                                                          # gtx_blocks_op.strand_op


class BlocksOp(ctypes.Structure):
    """gtx_blocks_op (include/gtx.h): one of genomic_blocks' six operations, select's flags, strand's -op"""
    _fields_ = [("kind", ctypes.c_int32), ("select", ctypes.c_int32), ("strand_op", ctypes.c_int32)]

    @classmethod
    def make(cls, kind, select=0, strand_op="+"):
        """kind: a word of BLOCKS_KINDS; strand_op: "+", "-" or "r" (either may be the number as it goes to the library)"""
        o = cls()
        o.kind = BLOCKS_KINDS.get(kind, kind)
        o.select = int(select)
        o.strand_op = BLOCKS_STRAND_OPS.get(strand_op, strand_op)
        return o


CONVERT_BED, CONVERT_REG = 0, 1                                                                      # gtx_convert_op.to


class ConvertOp(ctypes.Structure):
    """gtx_convert_op (include/gtx.h): the target format of genomic_convert, -chr and -c"""
    _fields_ = [("to", ctypes.c_int32), ("ucsc_names", ctypes.c_int32), ("color", ctypes.c_char_p)]

    @classmethod
    def make(cls, to, ucsc_names=False, color=None):
        """to: "bed" or "reg" (or the number as it goes to the library); color: bytes, str or None"""
        o = cls()
        o.to = {"bed": CONVERT_BED, "reg": CONVERT_REG}.get(to, to)
        o.ucsc_names = int(bool(ucsc_names))
        o.color = color.encode() if isinstance(color, str) else color
        return o


# name -> (restype, argtypes); must list every symbol include/gtx.h declares
# int sink(void *user, const char *text, size_t bytes) of gtx_window_lines / gtx_pair_lines
LINES_SINK = ctypes.CFUNCTYPE(ctypes.c_int, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_size_t)
LINES_TILE, LINES_MAX_NAME, E_SINK = 1024, 48, -5

ABI = {
    "gtx_version": (ctypes.c_int, []),
    "gtx_create": (ctypes.c_void_p, [ctypes.c_int]),
    "gtx_destroy": (None, [ctypes.c_void_p]),
    "gtx_last_error": (ctypes.c_char_p, [ctypes.c_void_p]),
    "gtx_set_stream": (ctypes.c_int, [ctypes.c_void_p, ctypes.c_void_p]),
    "gtx_sync": (ctypes.c_int, [ctypes.c_void_p]),
    "gtx_host_alloc": (ctypes.c_void_p, [ctypes.c_void_p, ctypes.c_size_t]),
    "gtx_host_free": (None, [ctypes.c_void_p, ctypes.c_void_p]),
    "gtx_set_refs": (ctypes.c_int, [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_int64, ctypes.c_int32]),
    "gtx_set_refs_ex": (ctypes.c_int, [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_int64, ctypes.c_int32, ctypes.c_uint32]),
    "gtx_n_refs": (ctypes.c_int64, [ctypes.c_void_p]),
    "gtx_count_begin": (ctypes.c_int, [ctypes.c_void_p]),
    "gtx_count_add": (ctypes.c_int, [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_int64, ctypes.c_uint32]),
    "gtx_count_end": (ctypes.c_int, [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p]),
    "gtx_count": (ctypes.c_int, [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_int64, ctypes.c_uint32,
                                 ctypes.c_void_p, ctypes.c_void_p]),
    "gtx_count_device": (ctypes.c_int, [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_int64, ctypes.c_uint32,
                                        ctypes.c_void_p]),
    "gtx_last_info": (ctypes.c_int, [ctypes.c_void_p, ctypes.c_void_p]),
    "gtx_coverage_begin": (ctypes.c_int, [ctypes.c_void_p]),
    "gtx_coverage_add": (ctypes.c_int, [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_int64, ctypes.c_uint32]),
    "gtx_coverage_end": (ctypes.c_int, [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p]),
    "gtx_coverage": (ctypes.c_int, [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_int64, ctypes.c_uint32,
                                    ctypes.c_void_p, ctypes.c_void_p]),
    "gtx_coverage_device": (ctypes.c_int, [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_int64, ctypes.c_uint32,
                                           ctypes.c_void_p]),
    "gtx_scan_n_windows": (ctypes.c_int64, [ctypes.c_int64, ctypes.c_int64, ctypes.c_int64]),
    "gtx_scan": (ctypes.c_int, [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_int64, ctypes.c_void_p,
                                ctypes.c_int32, ctypes.c_int32, ctypes.c_int32, ctypes.c_char, ctypes.c_uint32,
                                ctypes.c_void_p, ctypes.c_void_p]),
    "gtx_scan_device": (ctypes.c_int, [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_int64, ctypes.c_void_p,
                                       ctypes.c_int32, ctypes.c_int32, ctypes.c_int32, ctypes.c_char, ctypes.c_uint32,
                                       ctypes.c_void_p, ctypes.c_void_p]),
    "gtx_scan_begin": (ctypes.c_int, [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_int32, ctypes.c_int32, ctypes.c_int32, ctypes.c_char, ctypes.c_uint32,
                                      ctypes.c_int, ctypes.c_void_p]),
    "gtx_scan_add": (ctypes.c_int, [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_int64, ctypes.c_uint32]),
    "gtx_scan_add_text": (ctypes.c_int, [ctypes.c_void_p, ctypes.c_char_p, ctypes.c_size_t, ctypes.c_int64, ctypes.c_void_p, ctypes.c_uint32, ctypes.c_void_p]),
    "gtx_scan_end": (ctypes.c_int, [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p]),
    "gtx_scan_end_keep": (ctypes.c_int, [ctypes.c_void_p, ctypes.c_int, ctypes.c_void_p]),
    "gtx_scan_kept": (ctypes.c_int, [ctypes.c_void_p, ctypes.c_int, ctypes.c_void_p, ctypes.c_void_p]),
    "gtx_scan_drop": (ctypes.c_int, [ctypes.c_void_p, ctypes.c_int]),
    "gtx_window_select_limits": (ctypes.c_int, [ctypes.c_void_p, ctypes.c_void_p]),
    "gtx_window_select_device": (ctypes.c_int, [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_int32, ctypes.c_int64, ctypes.c_int32,
                                                ctypes.c_void_p, ctypes.c_int64, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p]),
    "gtx_window_select": (ctypes.c_int, [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_int32, ctypes.c_int64, ctypes.c_int32,
                                         ctypes.c_void_p, ctypes.c_int64, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p]),
    "gtx_window_refs": (ctypes.c_int, [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_int64, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_int32, ctypes.c_int32,
                                       ctypes.c_int32]),
    "gtx_window_filter_device": (ctypes.c_int, [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_int64, ctypes.c_uint64, ctypes.c_int64, ctypes.c_void_p,
                                                ctypes.c_void_p, ctypes.c_void_p]),
    "gtx_window_filter": (ctypes.c_int, [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_int64, ctypes.c_uint64, ctypes.c_int64, ctypes.c_void_p,
                                         ctypes.c_void_p, ctypes.c_void_p]),
    "gtx_scan_kept_read": (ctypes.c_int, [ctypes.c_void_p, ctypes.c_int, ctypes.c_void_p]),
    "gtx_peak_select_device": (ctypes.c_int, [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_int64, ctypes.c_int64, ctypes.c_int64,
                                              ctypes.c_int, ctypes.c_double, ctypes.c_int64, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p]),
    "gtx_peak_select": (ctypes.c_int, [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_int64, ctypes.c_int64, ctypes.c_int64,
                                       ctypes.c_int, ctypes.c_double, ctypes.c_int64, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p]),
    "gtx_lines_layout": (ctypes.c_int, [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_int32, ctypes.c_char_p, ctypes.c_void_p, ctypes.c_char_p, ctypes.c_int64,
                                        ctypes.c_int64]),
    "gtx_lines_max_bytes": (ctypes.c_int64, [ctypes.c_void_p]),
    "gtx_set_lines_chunk": (ctypes.c_int, [ctypes.c_void_p, ctypes.c_int64]),
    "gtx_window_lines_device": (ctypes.c_int, [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_int64, ctypes.c_int64, ctypes.c_int64, ctypes.c_int64, ctypes.c_void_p,
                                               ctypes.c_int64, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p]),
    "gtx_pair_lines_device": (ctypes.c_int, [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_int64, ctypes.c_int64, ctypes.c_int64, ctypes.c_void_p,
                                             ctypes.c_int64, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p]),
    "gtx_window_lines": (ctypes.c_int, [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_int64, ctypes.c_int64, ctypes.c_int64, LINES_SINK, ctypes.c_void_p,
                                        ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p]),
    "gtx_pair_lines": (ctypes.c_int, [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_int64, ctypes.c_int64, LINES_SINK, ctypes.c_void_p,
                                      ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p]),
    "gtx_window_filter_lines": (ctypes.c_int, [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_int64, ctypes.c_uint64, ctypes.c_int64, LINES_SINK, ctypes.c_void_p,
                                               ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p]),
    "gtx_sort": (ctypes.c_int, [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_int64, ctypes.c_int32, ctypes.c_void_p, ctypes.c_void_p]),
    "gtx_sort_device": (ctypes.c_int, [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_int64, ctypes.c_int32, ctypes.c_void_p, ctypes.c_void_p]),
    "gtx_link": (ctypes.c_int, [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_int64, ctypes.c_int64, ctypes.c_uint32,
                                ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p]),
    "gtx_link_device": (ctypes.c_int, [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_int64, ctypes.c_int64, ctypes.c_uint32,
                                       ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p]),
    "gtx_link_text_begin": (ctypes.c_int, [ctypes.c_void_p, ctypes.c_int32, ctypes.c_int, ctypes.c_int64]),
    "gtx_link_add_text": (ctypes.c_int, [ctypes.c_void_p, ctypes.c_char_p, ctypes.c_size_t, ctypes.c_int64, ctypes.c_void_p, ctypes.c_void_p]),
    "gtx_link_add": (ctypes.c_int, [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_int64]),
    "gtx_link_text_end": (ctypes.c_int, [ctypes.c_void_p, ctypes.c_int64, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p]),
    "gtx_adjacent": (ctypes.c_int, [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_int64, ctypes.c_int, ctypes.c_int, ctypes.c_void_p, ctypes.c_void_p]),
    "gtx_adjacent_device": (ctypes.c_int, [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_int64, ctypes.c_int, ctypes.c_int, ctypes.c_void_p,
                                           ctypes.c_void_p]),
    "gtx_gaps": (ctypes.c_int, [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_int64, ctypes.c_void_p, ctypes.c_int32, ctypes.c_int64, ctypes.c_void_p, ctypes.c_void_p,
                                ctypes.c_void_p, ctypes.c_void_p]),
    "gtx_gaps_device": (ctypes.c_int, [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_int64, ctypes.c_void_p, ctypes.c_int32, ctypes.c_int64, ctypes.c_void_p,
                                       ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p]),
    "gtx_group_count_add_text": (ctypes.c_int, [ctypes.c_void_p, ctypes.c_char_p, ctypes.c_size_t, ctypes.c_int64, ctypes.c_void_p, ctypes.c_uint32, ctypes.c_void_p]),
    "gtx_group_coverage_add_text": (ctypes.c_int, [ctypes.c_void_p, ctypes.c_char_p, ctypes.c_size_t, ctypes.c_int64, ctypes.c_void_p, ctypes.c_uint32, ctypes.c_void_p]),
    "gtx_group_text_result": (ctypes.c_int, [ctypes.c_void_p, ctypes.c_int, ctypes.c_void_p]),
    "gtx_group_create": (ctypes.c_void_p, [ctypes.c_int, ctypes.c_void_p]),
    "gtx_group_destroy": (None, [ctypes.c_void_p]),
    "gtx_group_size": (ctypes.c_int, [ctypes.c_void_p]),
    "gtx_group_ctx": (ctypes.c_void_p, [ctypes.c_void_p, ctypes.c_int]),
    "gtx_group_last_error": (ctypes.c_char_p, [ctypes.c_void_p]),
    "gtx_group_unique_id": (ctypes.c_int, [ctypes.c_void_p]),
    "gtx_group_create_rank": (ctypes.c_void_p, [ctypes.c_int, ctypes.c_int, ctypes.c_int, ctypes.c_void_p]),
    "gtx_group_rank": (ctypes.c_int, [ctypes.c_void_p]),
    "gtx_group_plan": (ctypes.c_int, [ctypes.c_void_p, ctypes.c_int64, ctypes.c_int64, ctypes.c_void_p, ctypes.c_int32, ctypes.c_int,
                                      ctypes.c_void_p, ctypes.c_void_p]),
    "gtx_group_count_device": (ctypes.c_int, [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_uint32, ctypes.c_void_p]),
    "gtx_group_scan_device": (ctypes.c_int, [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_int32,
                                             ctypes.c_int32, ctypes.c_int32, ctypes.c_char, ctypes.c_uint32, ctypes.c_void_p, ctypes.c_void_p]),
    "gtx_group_sync": (ctypes.c_int, [ctypes.c_void_p]),
    "gtx_group_wait_result": (ctypes.c_int, [ctypes.c_void_p]),
    "gtx_group_last_info": (ctypes.c_int, [ctypes.c_void_p, ctypes.c_void_p]),
    "gtx_group_assign": (ctypes.c_int, [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_int32, ctypes.c_void_p]),
    "gtx_lpt_assign": (None, [ctypes.c_void_p, ctypes.c_int32, ctypes.c_int, ctypes.c_void_p]),
    "gtx_group_set_refs": (ctypes.c_int, [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_int64, ctypes.c_int32, ctypes.c_uint32]),
    "gtx_group_count_begin": (ctypes.c_int, [ctypes.c_void_p]),
    "gtx_group_count_add": (ctypes.c_int, [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_int64, ctypes.c_uint32]),
    "gtx_group_count_end": (ctypes.c_int, [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p]),
    "gtx_group_coverage_begin": (ctypes.c_int, [ctypes.c_void_p]),
    "gtx_group_coverage_add": (ctypes.c_int, [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_int64, ctypes.c_uint32]),
    "gtx_group_coverage_end": (ctypes.c_int, [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p]),
    "gtx_group_scan": (ctypes.c_int, [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_int64, ctypes.c_void_p,
                                      ctypes.c_int32, ctypes.c_int32, ctypes.c_int32, ctypes.c_char, ctypes.c_uint32,
                                      ctypes.c_void_p, ctypes.c_void_p]),
    "gtx_group_member_reads": (ctypes.c_int, [ctypes.c_void_p, ctypes.c_void_p]),
    "gtx_set_ref_blocks": (ctypes.c_int, [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p]),
    "gtx_count_add_regions": (ctypes.c_int, [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_int64]),
    "gtx_group_set_ref_blocks": (ctypes.c_int, [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p]),
    "gtx_group_count_add_regions": (ctypes.c_int, [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_int64]),
    "gtx_count_add_text": (ctypes.c_int, [ctypes.c_void_p, ctypes.c_char_p, ctypes.c_size_t, ctypes.c_int64, ctypes.c_void_p, ctypes.c_uint32, ctypes.c_void_p]),
    "gtx_coverage_add_text": (ctypes.c_int, [ctypes.c_void_p, ctypes.c_char_p, ctypes.c_size_t, ctypes.c_int64, ctypes.c_void_p, ctypes.c_uint32, ctypes.c_void_p]),
    "gtx_text_result": (ctypes.c_int, [ctypes.c_void_p, ctypes.c_int, ctypes.c_void_p]),
    "gtx_subset_text": (ctypes.c_int, [ctypes.c_void_p, ctypes.c_char_p, ctypes.c_size_t, ctypes.c_int64, ctypes.c_void_p, ctypes.c_uint32, ctypes.c_void_p]),
    "gtx_subset_result": (ctypes.c_int, [ctypes.c_void_p, ctypes.c_int, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p]),
    "gtx_rewrite_text": (ctypes.c_int, [ctypes.c_void_p, ctypes.c_char_p, ctypes.c_size_t, ctypes.c_int64, ctypes.c_void_p, ctypes.c_void_p]),
    "gtx_rewrite_result": (ctypes.c_int, [ctypes.c_void_p, ctypes.c_int, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_size_t, ctypes.c_void_p, ctypes.c_void_p]),
    "gtx_rewrite_max_bytes": (ctypes.c_size_t, [ctypes.c_size_t, ctypes.c_int64]),
    "gtx_rewrite_limits": (ctypes.c_int, [ctypes.c_void_p, ctypes.c_void_p]),
    "gtx_convert_text": (ctypes.c_int, [ctypes.c_void_p, ctypes.c_char_p, ctypes.c_size_t, ctypes.c_int64, ctypes.c_void_p, ctypes.c_uint32, ctypes.c_void_p]),
    "gtx_convert_result": (ctypes.c_int, [ctypes.c_void_p, ctypes.c_int, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_size_t, ctypes.c_void_p, ctypes.c_void_p]),
    "gtx_convert_max_bytes": (ctypes.c_size_t, [ctypes.c_size_t, ctypes.c_int64, ctypes.c_void_p]),
    "gtx_convert_limits": (ctypes.c_int, [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p]),
    "gtx_windows_text": (ctypes.c_int, [ctypes.c_void_p, ctypes.c_char_p, ctypes.c_size_t, ctypes.c_int64, ctypes.c_void_p, ctypes.c_void_p]),
    "gtx_windows_result": (ctypes.c_int, [ctypes.c_void_p, ctypes.c_int, ctypes.c_void_p, LINES_SINK, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p]),
    "gtx_windows_limits": (ctypes.c_int, [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p]),
    "gtx_blocks_text": (ctypes.c_int, [ctypes.c_void_p, ctypes.c_char_p, ctypes.c_size_t, ctypes.c_int64, ctypes.c_void_p, ctypes.c_void_p]),
    "gtx_blocks_result": (ctypes.c_int, [ctypes.c_void_p, ctypes.c_int, ctypes.c_void_p, LINES_SINK, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p]),
    "gtx_blocks_max_bytes": (ctypes.c_size_t, [ctypes.c_size_t, ctypes.c_int64, ctypes.c_void_p]),
    "gtx_blocks_limits": (ctypes.c_int, [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p]),
    "gtx_set_ref_order": (ctypes.c_int, [ctypes.c_void_p, ctypes.c_void_p]),
    "gtx_set_join_buffer": (ctypes.c_int, [ctypes.c_void_p, ctypes.c_int64]),
    "gtx_join": (ctypes.c_int, [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_int64, ctypes.c_uint32,
                                ctypes.c_void_p, ctypes.c_void_p, ctypes.c_int64, ctypes.c_void_p]),
    "gtx_join_device": (ctypes.c_int, [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_int64, ctypes.c_uint32, ctypes.c_void_p, ctypes.c_void_p,
                                       ctypes.c_int64, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p]),
    "gtx_query_hits": (ctypes.c_int, [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_int64, ctypes.c_uint32,
                                      ctypes.c_void_p, ctypes.c_void_p]),
    "gtx_query_hits_device": (ctypes.c_int, [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_int64, ctypes.c_uint32, ctypes.c_void_p, ctypes.c_void_p]),
    "gtx_set_ref_strands": (ctypes.c_int, [ctypes.c_void_p, ctypes.c_void_p]),
    "gtx_join_offsets": (ctypes.c_int, [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_int64,
                                        ctypes.c_uint32, ctypes.c_int32, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_int64, ctypes.c_void_p,
                                        ctypes.c_void_p, ctypes.c_int64, ctypes.c_void_p, ctypes.c_void_p]),
    "gtx_pair_offsets_device": (ctypes.c_int, [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_int64, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_int64,
                                               ctypes.c_int32, ctypes.c_void_p, ctypes.c_void_p]),
    "gtx_pair_annotate_device": (ctypes.c_int, [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_int64, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_int64,
                                                ctypes.c_int64, ctypes.c_int32, ctypes.c_int32, ctypes.c_int32, ctypes.c_void_p, ctypes.c_void_p,
                                                ctypes.c_void_p, ctypes.c_int64, ctypes.c_void_p]),
    "gtx_join_annotate": (ctypes.c_int, [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_int64, ctypes.c_uint32, ctypes.c_int64, ctypes.c_int32,
                                         ctypes.c_int32, ctypes.c_int32, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_int64,
                                         ctypes.c_void_p, ctypes.c_void_p]),
    "gtx_set_signal_bins": (ctypes.c_int, [ctypes.c_void_p, ctypes.c_double, ctypes.c_double, ctypes.c_int64, ctypes.c_void_p]),
    "gtx_signal_bins": (ctypes.c_int, [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_int64,
                                       ctypes.c_uint32, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p]),
    "gtx_signal_bins_device": (ctypes.c_int, [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_int64, ctypes.c_uint32, ctypes.c_void_p,
                                              ctypes.c_void_p, ctypes.c_void_p]),
    "gtx_profile_enable": (ctypes.c_int, [ctypes.c_void_p, ctypes.c_int]),
    "gtx_profile_last": (ctypes.c_int, [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p]),
    "gtx_profile_count": (ctypes.c_int, [ctypes.c_void_p]),
    "gtx_profile_read": (ctypes.c_int, [ctypes.c_void_p, ctypes.c_int, ctypes.c_void_p, ctypes.c_void_p]),
}


def load():
    """dlopen libgtx.so and type its entry points; raises if the library has not been built."""
    global _lib
    if _lib is None:
        if not os.path.exists(LIB_PATH):
            raise GtxError("%s not found: build it with `make -C %s` (python __graft_entry__.py does)"
                           % (LIB_PATH, os.path.dirname(LIB_PATH)))
        # One HIP runtime per process: PyTorch bundles its own libamdhip64.so.7 (same soname as
        # /opt/rocm's).  If torch is going to be used for device buffers / torch.distributed, its
        # runtime has to be the one that is loaded first, otherwise torch finds no GPU.
        if not os.environ.get("GTX_NO_TORCH"):
            try:
                import torch  # noqa: F401
            except ImportError:
                pass
        lib = ctypes.CDLL(LIB_PATH)
        for name, (res, args) in ABI.items():
            fn = getattr(lib, name)
            fn.restype = res
            fn.argtypes = args
        _lib = lib
    return _lib


def _ptr(a):
    if a is None:
        return None
    if isinstance(a, np.ndarray):
        return a.ctypes.data_as(ctypes.c_void_p)
    return ctypes.c_void_p(int(a))          # raw device/host address


def _strands(strand):
    """'+' / '-' (str, bytes or characters), or 0 / 1, as the int8 characters of the C ABI"""
    if isinstance(strand, (str, bytes)):
        a = np.frombuffer(strand.encode() if isinstance(strand, str) else strand, dtype=np.int8)
    else:
        a = np.asarray(strand)
        if a.dtype.kind in "US":
            a = np.frombuffer("".join(a.tolist()).encode(), dtype=np.int8)
        else:
            a = np.where(a.astype(np.int64) != 0, ord("-"), ord("+")).astype(np.int8)
    return np.ascontiguousarray(a, dtype=np.int8)


def _triples(a):
    a = np.ascontiguousarray(a, dtype=np.int32)
    if a.ndim != 2 or a.shape[1] != 3:
        raise ValueError("expected an (n, 3) int32 array of (class, start, end)")
    return a


def scan_layout(class_len, win_step, win_size):
    """(offsets, total) of the concatenated per-class window vector gtx_scan fills."""
    lib = load()
    off, tot = [], 0
    for ln in class_len:
        off.append(tot)
        tot += lib.gtx_scan_n_windows(int(ln), int(win_step), int(win_size))
    return np.asarray(off, dtype=np.int64), tot


def rewrite_limits():
    """(tile, stage) of gtx_rewrite_limits: lines per tile of the rewrite's passes; bytes of a tile's text, and of its output,
    that the stage holds"""
    t, b = ctypes.c_int32(), ctypes.c_int32()
    load().gtx_rewrite_limits(ctypes.byref(t), ctypes.byref(b))
    return int(t.value), int(b.value)


def convert_limits():
    """(tile, stage, max_color) of gtx_convert_limits: lines per tile of the conversion's passes; bytes of a tile's output that the
    stage holds; the longest colour"""
    t, b, m = ctypes.c_int32(), ctypes.c_int32(), ctypes.c_int32()
    load().gtx_convert_limits(ctypes.byref(t), ctypes.byref(b), ctypes.byref(m))
    return int(t.value), int(b.value), int(m.value)


def blocks_limits():
    """(tile, stage, max_blocks) of gtx_blocks_limits: lines per tile of the block operations' plan and one-line emit; bytes of such
    a tile's output that the stage holds; the blocks of a plain 12-column line"""
    t, b, m = ctypes.c_int32(), ctypes.c_int32(), ctypes.c_int32()
    load().gtx_blocks_limits(ctypes.byref(t), ctypes.byref(b), ctypes.byref(m))
    return int(t.value), int(b.value), int(m.value)


def windows_limits():
    """(line_tile, out_tile, max_fixed) of gtx_windows_limits: lines per tile of the sliding windows' plan, windows per output tile
    of their emit pass, and the longest fixed part (column 1, two tabs, the tail, the newline) of a line the device takes"""
    t, w, f = ctypes.c_int32(), ctypes.c_int32(), ctypes.c_int32()
    load().gtx_windows_limits(ctypes.byref(t), ctypes.byref(w), ctypes.byref(f))
    return int(t.value), int(w.value), int(f.value)


def window_select_limits():
    """(tile, lds_max_w) of gtx_window_select_limits: windows per tile of the selection's passes; the largest window size whose
    tables sit in LDS with four tested vectors and controls"""
    t, w = ctypes.c_int32(), ctypes.c_int32()
    load().gtx_window_select_limits(ctypes.byref(t), ctypes.byref(w))
    return int(t.value), int(w.value)


def _text_format(sam, fmt=None):
    """the format flag of a text block.  fmt, when given, is the flag as it goes to the library (0, TEXT_SAM, TEXT_GFF).  Else `sam`
    decides as it always did -- any true value: SAM alignments -- except that one of the two format flags stands for itself, so that
    a caller with one positional argument for the format can pass TEXT_GFF."""
    if fmt is not None:
        return int(fmt)
    if not isinstance(sam, (bool, np.bool_)) and isinstance(sam, (int, np.integer)) and int(sam) in (TEXT_SAM, TEXT_GFF):
        return int(sam)
    return TEXT_SAM if sam else 0


def _two_in_flight(blocks, send, collect):
    """The loop of the calls that hand a block of text over under a ticket and fetch its result later: send(text) -> ticket for every
    block, collect(text, ticket) -> the block's result, two tickets in flight, the results in block order.  When either raises a
    GtxError the blocks still in flight are fetched to be forgotten (collect(text, ticket, drop=True); the block whose call failed
    is dropped by that call itself), so that the engine holds no block of the call, and the error is raised again."""
    tickets, results = [], []
    try:
        for text in blocks:
            if len(tickets) == 2:
                results.append(collect(*tickets.pop(0)))
            tickets.append((text, send(text)))
        while tickets:
            results.append(collect(*tickets.pop(0)))
    except GtxError:
        for x in tickets:
            collect(*x, drop=True)
        raise
    return results


def _guarded_out(cap, guard):
    """a caller's buffer of cap bytes with `guard` bytes of 0xA5 behind it, and intact(n): whether the bytes behind the 16-byte unit
    that a text of n bytes ends in are still what they were"""
    out = ctypes.create_string_buffer(b"\xa5" * (cap + guard), cap + guard)

    def intact(n):
        behind = (n + 15) // 16 * 16
        return out.raw[behind:] == b"\xa5" * (cap + guard - behind)
    return out, intact


class Engine:
    """One context on one GPU (one per process in multi-GPU runs)."""

    def __init__(self, device=0):
        self.lib = load()
        self.ctx = self.lib.gtx_create(int(device))
        if not self.ctx:
            raise GtxError(self.lib.gtx_last_error(None).decode())
        self.n_refs = 0
        self._sig_bins = 0

    def close(self):
        if getattr(self, "ctx", None):
            self.lib.gtx_destroy(self.ctx)
            self.ctx = None

    def __del__(self):
        self.close()

    def _chk(self, rc):
        if rc != 0:
            raise GtxError("gtx error %d: %s" % (rc, self.lib.gtx_last_error(self.ctx).decode()))

    def set_stream(self, stream_handle):
        self._chk(self.lib.gtx_set_stream(self.ctx, ctypes.c_void_p(int(stream_handle))))

    def sync(self):
        self._chk(self.lib.gtx_sync(self.ctx))
        self._link_infos = []

    def pinned_array(self, shape, dtype=np.int32):
        """numpy array over page-locked memory from gtx_host_alloc (the DMA engine reads it without a staging copy).
        The memory lives until free_pinned(array) or the end of the process."""
        n = int(np.prod(shape)) * np.dtype(dtype).itemsize
        p = self.lib.gtx_host_alloc(self.ctx, max(n, 1))
        if not p:
            raise GtxError(self.lib.gtx_last_error(self.ctx).decode())
        buf = (ctypes.c_char * max(n, 1)).from_address(p)
        a = np.frombuffer(buf, dtype=dtype, count=int(np.prod(shape))).reshape(shape)
        self._pinned = getattr(self, "_pinned", {})
        self._pinned[a.ctypes.data] = p
        return a

    def free_pinned(self, a):
        p = getattr(self, "_pinned", {}).pop(a.ctypes.data, None)
        if p:
            self.lib.gtx_host_free(self.ctx, ctypes.c_void_p(p))

    def set_refs(self, refs, n_classes=0, flags=0):
        refs = _triples(refs)
        self._chk(self.lib.gtx_set_refs_ex(self.ctx, _ptr(refs), refs.shape[0], int(n_classes), int(flags)))
        self.n_refs = refs.shape[0]

    def set_ref_blocks(self, first=None, blocks=None):
        """gtx_set_ref_blocks: region k's intervals are blocks[first[k]:first[k+1]] ((start, stop) rows); None: envelopes only."""
        if first is None:
            self._chk(self.lib.gtx_set_ref_blocks(self.ctx, None, None))
            return
        first = np.ascontiguousarray(first, dtype=np.int64)
        blocks = np.ascontiguousarray(blocks, dtype=np.int32).reshape(-1, 2)
        if len(first) != self.n_refs + 1 or first[-1] != len(blocks):
            raise GtxError("set_ref_blocks: first must have n_refs + 1 entries and end at len(blocks)")
        self._chk(self.lib.gtx_set_ref_blocks(self.ctx, _ptr(first), _ptr(blocks)))

    def count_stream(self, batches, flags=READS_SORTED, regions=()):
        """gtx_count_begin / _add per (reads, weights) batch / _add_regions per (env_triples, weights, first, blocks) / _end."""
        self._chk(self.lib.gtx_count_begin(self.ctx))
        for reads, w in batches:
            reads = _triples(reads)
            w = None if w is None else np.ascontiguousarray(w, dtype=np.int32)
            self._chk(self.lib.gtx_count_add(self.ctx, _ptr(reads), _ptr(w), reads.shape[0], int(flags)))
        for env, w, first, blocks in regions:
            env = _triples(env)
            w = None if w is None else np.ascontiguousarray(w, dtype=np.int32)
            first = np.ascontiguousarray(first, dtype=np.int64)
            blocks = np.ascontiguousarray(blocks, dtype=np.int32).reshape(-1, 2)
            if len(first) != env.shape[0] + 1 or first[-1] != len(blocks):
                raise GtxError("count_stream: first must have n + 1 entries and end at len(blocks)")
            self._chk(self.lib.gtx_count_add_regions(self.ctx, _ptr(env), _ptr(w), _ptr(first), _ptr(blocks), env.shape[0]))
        hits = np.zeros(max(self.n_refs, 1), dtype=np.uint64)
        info = CountInfo()
        self._chk(self.lib.gtx_count_end(self.ctx, _ptr(hits), ctypes.byref(info)))
        return hits[:self.n_refs], info.as_dict()

    def _reduce_text(self, which, blocks, rules, flags, sam, fmt=None):
        begin, add, end = (getattr(self.lib, "gtx_%s_%s" % (which, f)) for f in ("begin", "add_text", "end"))
        blocks = list(blocks)
        per_block = rules if isinstance(rules, (list, tuple)) else [rules] * len(blocks)
        if len(per_block) != len(blocks):
            raise GtxError("%s_text: one TextRules per block" % which)
        self._chk(begin(self.ctx))
        verdicts = []
        for text, r in zip(blocks, per_block):
            t = ctypes.c_int(-1)
            self._chk(add(self.ctx, text, len(text), text.count(b"\n"), ctypes.byref(r), int(flags) | _text_format(sam, fmt), ctypes.byref(t)))
            redo = ctypes.c_int(0)
            self._chk(self.lib.gtx_text_result(self.ctx, t.value, ctypes.byref(redo)))
            verdicts.append(redo.value)
        out = np.zeros(max(self.n_refs, 1), dtype=np.uint64)
        info = CountInfo()
        self._chk(end(self.ctx, _ptr(out), ctypes.byref(info)))
        return out[:self.n_refs], info.as_dict(), verdicts

    def count_text(self, blocks, rules, flags=READS_SORTED, sam=False, fmt=None):
        """gtx_count_begin / gtx_count_add_text per block of text (bytes of complete lines) / gtx_count_end; sam=True: SAM alignments
        (GTX_TEXT_SAM); fmt=TEXT_GFF: GFF / GTF features (fmt: the format flag as it goes to the library).  rules: one TextRules for every block, or a list with one per block (each block's own seam key).
        Returns (hits, info, needs_host verdict per block) -- a block that comes back was not counted."""
        return self._reduce_text("count", blocks, rules, flags, sam, fmt)

    def coverage_text(self, blocks, rules, flags=READS_SORTED, sam=False, fmt=None):
        """the same through gtx_coverage_begin / gtx_coverage_add_text / gtx_coverage_end: (coverage, info, verdicts)"""
        return self._reduce_text("coverage", blocks, rules, flags, sam, fmt)

    def _result_into(self, result, t, cap, guard, drop):
        """gtx_*_result(ctx, t, &needs_host, out, cap, &bytes, &lines) into a guarded buffer: (needs_host, the text, the lines,
        whether the guard is whole); drop: the block is fetched to be forgotten, whatever the call says"""
        redo, nb, ns = ctypes.c_int(0), ctypes.c_size_t(0), ctypes.c_int64(0)
        out, intact = _guarded_out(cap, guard)
        rc = result(self.ctx, t, ctypes.byref(redo), out, cap, ctypes.byref(nb), ctypes.byref(ns))
        if drop:
            return None
        self._chk(rc)
        return redo.value, out.raw[:nb.value], ns.value, intact(nb.value)

    def _result_sink(self, name, result, t, drop, refuse=lambda: False):
        """gtx_*_result(ctx, t, &needs_host, sink, user, &lines, &bytes) into a sink that collects the text: (needs_host, the text,
        the lines, the number of sink calls).  The sink refuses a call when refuse() says so, and every call of a dropped block."""
        parts, calls = [], [0]

        def take(user, p, n):
            calls[0] += 1
            if drop or refuse():
                return 1
            parts.append(ctypes.string_at(p, n))
            return 0
        redo, nl, nb = ctypes.c_int(0), ctypes.c_int64(0), ctypes.c_int64(0)
        rc = result(self.ctx, t, ctypes.byref(redo), LINES_SINK(take), None, ctypes.byref(nl), ctypes.byref(nb))
        if drop:
            return None
        self._chk(rc)
        out = b"".join(parts)
        if nb.value != len(out):
            raise GtxError("%s: n_bytes %d, the sink was given %d" % (name, nb.value, len(out)))
        return redo.value, out, nl.value, calls[0]

    def subset_text(self, blocks, rules, flags=0):
        """gtx_subset_text / gtx_subset_result per block of text (bytes of complete lines), two blocks in flight: per block
        (needs_host, the selected text, the number of selected lines); a block that comes back selected nothing."""
        def send(text):
            t = ctypes.c_int(-1)
            self._chk(self.lib.gtx_subset_text(self.ctx, text, len(text), text.count(b"\n"), ctypes.byref(rules), int(flags), ctypes.byref(t)))
            return t.value

        def collect(text, t, drop=False):
            redo, nb, ns = ctypes.c_int(0), ctypes.c_size_t(0), ctypes.c_int64(0)
            out = ctypes.create_string_buffer(max(len(text), 1))
            rc = self.lib.gtx_subset_result(self.ctx, t, ctypes.byref(redo), out, ctypes.byref(nb), ctypes.byref(ns))
            if drop:
                return None
            self._chk(rc)
            return redo.value, out.raw[:nb.value], ns.value
        return _two_in_flight(blocks, send, collect)

    def rewrite_text(self, blocks, op, guard=64):
        """gtx_rewrite_text / gtx_rewrite_result per block of text (bytes of complete lines), two blocks in flight: per block
        (needs_host, the printed text, the number of printed lines, whether the bytes behind the text's 16-byte unit were left
        alone).  out is gtx_rewrite_max_bytes long, rounded up to 16, with `guard` bytes of 0xA5 behind it: the caller's buffer, not the
        device buffer the kernels store into."""
        def send(text):
            t = ctypes.c_int(-1)
            self._chk(self.lib.gtx_rewrite_text(self.ctx, text, len(text), text.count(b"\n"), ctypes.byref(op), ctypes.byref(t)))
            return t.value

        def collect(text, t, drop=False):
            cap = (int(self.lib.gtx_rewrite_max_bytes(len(text), text.count(b"\n"))) + 15) // 16 * 16
            return self._result_into(self.lib.gtx_rewrite_result, t, cap, guard, drop)
        return _two_in_flight(blocks, send, collect)

    def convert_text(self, blocks, op, fmt=0, guard=64):
        """gtx_convert_text / gtx_convert_result per block of text (bytes of complete lines; fmt: 0 for BED, TEXT_SAM or TEXT_GFF), two
        blocks in flight: per block (needs_host, the printed text, the number of printed lines, whether the bytes behind the text's
        16-byte unit were left alone).  out is gtx_convert_max_bytes long, rounded up to 16, with `guard` bytes of 0xA5 behind it:
        the caller's buffer, not the device buffer the kernels store into."""
        def send(text):
            t = ctypes.c_int(-1)
            self._chk(self.lib.gtx_convert_text(self.ctx, text, len(text), text.count(b"\n"), ctypes.byref(op), int(fmt), ctypes.byref(t)))
            return t.value

        def collect(text, t, drop=False):
            cap = (int(self.lib.gtx_convert_max_bytes(len(text), text.count(b"\n"), ctypes.byref(op))) + 15) // 16 * 16
            return self._result_into(self.lib.gtx_convert_result, t, cap, guard, drop)
        return _two_in_flight(blocks, send, collect)

    def blocks_text(self, blocks, op, chunk=None):
        """gtx_blocks_text / gtx_blocks_result per block of text (bytes of complete lines), two blocks in flight: per block
        (needs_host, the printed text, the number of printed lines, the number of sink calls).  chunk: gtx_set_lines_chunk first."""
        if chunk is not None:
            self.set_lines_chunk(chunk)

        def send(text):
            t = ctypes.c_int(-1)
            self._chk(self.lib.gtx_blocks_text(self.ctx, text, len(text), text.count(b"\n"), ctypes.byref(op), ctypes.byref(t)))
            return t.value

        def collect(text, t, drop=False):
            return self._result_sink("gtx_blocks_result", self.lib.gtx_blocks_result, t, drop)
        return _two_in_flight(blocks, send, collect)

    def windows_text(self, blocks, op, chunk=None, refuse_at=None):
        """gtx_windows_text / gtx_windows_result per block of text (bytes of complete lines), two blocks in flight: per block
        (needs_host, the windows' text, the number of windows, the number of sink calls).  chunk: gtx_set_lines_chunk first.
        refuse_at: the sink refuses its refuse_at-th call (counted from 1 over all blocks): the blocks still in flight are dropped
        and the GtxError of GTX_E_SINK is raised."""
        if chunk is not None:
            self.set_lines_chunk(chunk)
        calls = [0]

        def refuse():
            calls[0] += 1
            return calls[0] == refuse_at

        def send(text):
            t = ctypes.c_int(-1)
            self._chk(self.lib.gtx_windows_text(self.ctx, text, len(text), text.count(b"\n"), ctypes.byref(op), ctypes.byref(t)))
            return t.value

        def collect(text, t, drop=False):
            return self._result_sink("gtx_windows_result", self.lib.gtx_windows_result, t, drop, refuse)
        return _two_in_flight(blocks, send, collect)

    def count(self, reads, weights=None, flags=READS_SORTED):
        reads = _triples(reads)
        w = None if weights is None else np.ascontiguousarray(weights, dtype=np.int32)
        hits = np.zeros(max(self.n_refs, 1), dtype=np.uint64)
        info = CountInfo()
        self._chk(self.lib.gtx_count(self.ctx, _ptr(reads), _ptr(w), reads.shape[0], int(flags), _ptr(hits), ctypes.byref(info)))
        return hits[:self.n_refs], info.as_dict()

    def count_device(self, d_reads, n_reads, d_hits, d_weights=None, flags=READS_SORTED):
        """reads/weights/hits are raw device addresses (e.g. torch tensor .data_ptr()); asynchronous."""
        self._chk(self.lib.gtx_count_device(self.ctx, _ptr(d_reads), _ptr(d_weights), int(n_reads), int(flags), _ptr(d_hits)))

    def set_ref_order(self, key=None):
        """gtx_set_ref_order: pairs of a query come out in ascending (key[k], k); None: ordinal order."""
        if key is None:
            self._chk(self.lib.gtx_set_ref_order(self.ctx, None))
            return
        key = np.ascontiguousarray(key, dtype=np.int64)
        if len(key) != self.n_refs:
            raise GtxError("set_ref_order: one key per reference region")
        self._chk(self.lib.gtx_set_ref_order(self.ctx, _ptr(key)))

    def set_join_buffer(self, max_pairs):
        self._chk(self.lib.gtx_set_join_buffer(self.ctx, int(max_pairs)))

    def join(self, reads, flags=0, first=None, blocks=None, capacity=None):
        """gtx_join: (offsets [n+1] int64, pairs int32, info); query i's reference ordinals are pairs[offsets[i]:offsets[i+1]].
        first / blocks: the intervals of multi-interval queries (as set_ref_blocks).  capacity: room for pairs (None: all of them,
        found by a first call with no room)."""
        reads = _triples(reads)
        n = reads.shape[0]
        if first is not None:
            first = np.ascontiguousarray(first, dtype=np.int64)
            blocks = np.ascontiguousarray(blocks, dtype=np.int32).reshape(-1, 2)
            if len(first) != n + 1 or first[-1] != len(blocks):
                raise GtxError("join: first must have n + 1 entries and end at len(blocks)")
        off = np.zeros(n + 1, dtype=np.int64)
        info = CountInfo()
        if capacity is None:
            self._chk(self.lib.gtx_join(self.ctx, _ptr(reads), _ptr(first), _ptr(blocks), n, int(flags), _ptr(off), None, 0, ctypes.byref(info)))
            capacity = int(off[-1])
        pairs = np.zeros(max(int(capacity), 1), dtype=np.int32)
        self._chk(self.lib.gtx_join(self.ctx, _ptr(reads), _ptr(first), _ptr(blocks), n, int(flags), _ptr(off), _ptr(pairs), int(capacity),
                                    ctypes.byref(info)))
        return off, pairs[:min(int(capacity), int(off[-1]))], info.as_dict()

    def join_device(self, d_reads, n_reads, d_offsets, d_pairs, capacity, flags=0):
        """gtx_join_device on raw device addresses: (total pairs, queries done, info)."""
        tot, done = ctypes.c_int64(0), ctypes.c_int64(0)
        info = CountInfo()
        self._chk(self.lib.gtx_join_device(self.ctx, _ptr(d_reads), int(n_reads), int(flags), _ptr(d_offsets), _ptr(d_pairs), int(capacity),
                                           ctypes.byref(tot), ctypes.byref(done), ctypes.byref(info)))
        return tot.value, done.value, info.as_dict()

    def query_hits(self, reads, flags=0, first=None, blocks=None):
        """gtx_query_hits: (hits [n] uint32, info); hits[i] = the reference regions query i overlaps = the length of its segment
        in join() with the same arguments."""
        reads = _triples(reads)
        n = reads.shape[0]
        if first is not None:
            first = np.ascontiguousarray(first, dtype=np.int64)
            blocks = np.ascontiguousarray(blocks, dtype=np.int32).reshape(-1)
            if first.shape[0] != n + 1 or int(first[-1]) * 2 != blocks.shape[0]:
                raise GtxError("query_hits: first must have n + 1 entries and end at len(blocks)")
        hits = np.zeros(n, dtype=np.uint32)
        info = CountInfo()
        self._chk(self.lib.gtx_query_hits(self.ctx, _ptr(reads), _ptr(first), _ptr(blocks), n, int(flags), _ptr(hits), ctypes.byref(info)))
        return hits, info.as_dict()

    def query_hits_device(self, d_reads, n_reads, d_hits, flags=0):
        """gtx_query_hits_device on raw device addresses: info."""
        info = CountInfo()
        self._chk(self.lib.gtx_query_hits_device(self.ctx, _ptr(d_reads), int(n_reads), int(flags), _ptr(d_hits), ctypes.byref(info)))
        return info.as_dict()

    def set_ref_strands(self, strand=None):
        """gtx_set_ref_strands: one of '+' / '-' (or 0 '+', 1 '-') per reference region; None: all '+'."""
        if strand is None:
            self._chk(self.lib.gtx_set_ref_strands(self.ctx, None))
            return
        strand = _strands(strand)
        if len(strand) != self.n_refs:
            raise GtxError("set_ref_strands: one strand per reference region")
        self._chk(self.lib.gtx_set_ref_strands(self.ctx, _ptr(strand)))

    def join_offsets(self, reads, op="5p", flags=0, first=None, blocks=None, strands=None):
        """gtx_join_offsets: (offsets [n+1], pairs, entry offsets [pairs+1], entries [E, 2] int64, first inverted pair, info).
        op: "1", "2", "5p", "3p" (or its GTX_OFFSET_* code); strands: the queries' (GTX_OFFSET_FROM_QUERY)."""
        reads = _triples(reads)
        n = reads.shape[0]
        code = OFFSET_OPS[op] if isinstance(op, str) else int(op)
        if first is not None:
            first = np.ascontiguousarray(first, dtype=np.int64)
            blocks = np.ascontiguousarray(blocks, dtype=np.int32).reshape(-1, 2)
            if len(first) != n + 1 or first[-1] != len(blocks):
                raise GtxError("join_offsets: first must have n + 1 entries and end at len(blocks)")
        st = None if strands is None else _strands(strands)
        off = np.zeros(n + 1, dtype=np.int64)
        eoff = np.zeros(1, dtype=np.int64)
        inv = ctypes.c_int64(-1)
        info = CountInfo()

        def call(pairs, cap, eoff, entries, ecap):
            self._chk(self.lib.gtx_join_offsets(self.ctx, _ptr(reads), _ptr(first), _ptr(blocks), _ptr(st), n, int(flags), code, _ptr(off),
                                                _ptr(pairs), int(cap), _ptr(eoff), _ptr(entries), int(ecap), ctypes.byref(inv), ctypes.byref(info)))
        call(None, 0, None, None, 0)                                           # sizes: the pairs, then their entries
        cap = int(off[-1])
        pairs = np.zeros(max(cap, 1), dtype=np.int32)
        eoff = np.zeros(cap + 1, dtype=np.int64)
        call(pairs, cap, eoff, None, 0)
        ecap = int(eoff[-1])
        entries = np.zeros((max(ecap, 1), 2), dtype=np.int64)
        call(pairs, cap, eoff, entries, ecap)
        return off, pairs[:cap], eoff, entries[:ecap], inv.value, info.as_dict()

    def pair_offsets_device(self, d_reads, n_reads, d_offsets, d_pairs, n_pairs, d_out, op="5p"):
        """gtx_pair_offsets_device on raw device addresses (the pairs gtx_join_device left): the first inverted pair (-1: none)."""
        code = OFFSET_OPS[op] if isinstance(op, str) else int(op)
        inv = ctypes.c_int64(-1)
        self._chk(self.lib.gtx_pair_offsets_device(self.ctx, _ptr(d_reads), int(n_reads), _ptr(d_offsets), _ptr(d_pairs), int(n_pairs), code,
                                                   _ptr(d_out), ctypes.byref(inv)))
        return inv.value

    def pair_annotate_device(self, d_reads, n_reads, d_offsets, d_pairs, n_pairs, n_primary, d_kept_offsets, d_kept_ref, d_kept_value, capacity,
                             mode=ANNOTATE_CENTER, op_primary="5p", op_rest="3p"):
        """gtx_pair_annotate_device on raw device addresses (the pairs gtx_join_device left): the number of kept pairs, whatever
        the capacity."""
        kept = ctypes.c_int64(0)
        self._chk(self.lib.gtx_pair_annotate_device(self.ctx, _ptr(d_reads), int(n_reads), _ptr(d_offsets), _ptr(d_pairs), int(n_pairs),
                                                    int(n_primary), OFFSET_OPS[op_primary], OFFSET_OPS[op_rest], int(mode), _ptr(d_kept_offsets),
                                                    _ptr(d_kept_ref), _ptr(d_kept_value), int(capacity), ctypes.byref(kept)))
        return kept.value

    def join_annotate(self, reads, n_primary, mode=ANNOTATE_CENTER, flags=0, op_primary="5p", op_rest="3p", capacity=None):
        """gtx_join_annotate: (kept offsets [n+1] int64, kept ordinals int32, kept values int64, pairs of the join, info).  capacity:
        room for kept pairs (None: all of them, found by a first call with no room)."""
        reads = _triples(reads)
        n = reads.shape[0]
        koff = np.zeros(n + 1, dtype=np.int64)
        npairs = ctypes.c_int64(0)
        info = CountInfo()

        def call(ref, val, cap):
            self._chk(self.lib.gtx_join_annotate(self.ctx, _ptr(reads), n, int(flags), int(n_primary), OFFSET_OPS[op_primary], OFFSET_OPS[op_rest],
                                                 int(mode), _ptr(koff), _ptr(ref), _ptr(val), int(cap), ctypes.byref(npairs), ctypes.byref(info)))
        if capacity is None:
            call(None, None, 0)
            capacity = int(koff[-1])
        ref = np.zeros(max(int(capacity), 1), dtype=np.int32)
        val = np.zeros(max(int(capacity), 1), dtype=np.int64)
        call(ref, val, capacity)
        k = min(int(capacity), int(koff[-1]))
        return koff, ref[:k], val[:k], npairs.value, info.as_dict()

    def set_signal_bins(self, bin_min, bin_max, n_bins, ref_len=None):
        """gtx_set_signal_bins: the bin geometry; ref_len: one length per reference region (None: 1)."""
        rl = None
        if ref_len is not None:
            rl = np.ascontiguousarray(ref_len, dtype=np.int64)
            if len(rl) != self.n_refs:
                raise GtxError("set_signal_bins: one length per reference region")
        self._chk(self.lib.gtx_set_signal_bins(self.ctx, float(bin_min), float(bin_max), int(n_bins), _ptr(rl)))
        self._sig_bins = int(n_bins)

    def signal_bins(self, reads, weights=None, flags=0, first=None, blocks=None):
        """gtx_signal_bins: (bins int64 -- [n_bins], or [n_refs, n_bins] with SIGNAL_PER_REF --, first inverted read, info).
        weights: int64 per read (None: 1); first / blocks: the intervals of multi-interval reads (as join)."""
        reads = _triples(reads)
        n = reads.shape[0]
        if first is not None:
            first = np.ascontiguousarray(first, dtype=np.int64)
            blocks = np.ascontiguousarray(blocks, dtype=np.int32).reshape(-1, 2)
            if len(first) != n + 1 or first[-1] != len(blocks):
                raise GtxError("signal_bins: first must have n + 1 entries and end at len(blocks)")
        w = None if weights is None else np.ascontiguousarray(weights, dtype=np.int64)
        if w is not None and len(w) != n:
            raise GtxError("signal_bins: one weight per read")
        rows = self.n_refs if flags & SIGNAL_PER_REF else 1
        bins = np.zeros(max(rows * self._sig_bins, 1), dtype=np.int64)
        inv = ctypes.c_int64(-1)
        info = SignalInfo()
        self._chk(self.lib.gtx_signal_bins(self.ctx, _ptr(reads), _ptr(first), _ptr(blocks), _ptr(w), n, int(flags), _ptr(bins),
                                           ctypes.byref(inv), ctypes.byref(info)))
        bins = bins[:rows * self._sig_bins]
        return (bins.reshape(rows, self._sig_bins) if flags & SIGNAL_PER_REF else bins), inv.value, info.as_dict()

    def signal_bins_device(self, d_reads, n_reads, d_bins, d_weights=None, flags=0):
        """gtx_signal_bins_device on raw device addresses (d_bins int64, added to): (first inverted read, info)."""
        inv = ctypes.c_int64(-1)
        info = SignalInfo()
        self._chk(self.lib.gtx_signal_bins_device(self.ctx, _ptr(d_reads), _ptr(d_weights), int(n_reads), int(flags), _ptr(d_bins),
                                                  ctypes.byref(inv), ctypes.byref(info)))
        return inv.value, info.as_dict()

    def coverage(self, reads, weights=None, flags=READS_SORTED):
        reads = _triples(reads)
        w = None if weights is None else np.ascontiguousarray(weights, dtype=np.int32)
        cov = np.zeros(max(self.n_refs, 1), dtype=np.uint64)
        info = CountInfo()
        self._chk(self.lib.gtx_coverage(self.ctx, _ptr(reads), _ptr(w), reads.shape[0], int(flags), _ptr(cov), ctypes.byref(info)))
        return cov[:self.n_refs], info.as_dict()

    def coverage_device(self, d_reads, n_reads, d_cov, d_weights=None, flags=READS_SORTED):
        self._chk(self.lib.gtx_coverage_device(self.ctx, _ptr(d_reads), _ptr(d_weights), int(n_reads), int(flags), _ptr(d_cov)))

    def last_info(self):
        info = CountInfo()
        self._chk(self.lib.gtx_last_info(self.ctx, ctypes.byref(info)))
        return info.as_dict()

    def sort(self, reads, n_classes, want_sorted=True):
        """gtx_sort: (order, sorted triples or None) under (class, start, stop descending, input order)"""
        reads = _triples(reads)
        order = np.empty(reads.shape[0], dtype=np.uint32)
        out = np.empty_like(reads) if want_sorted else None
        self._chk(self.lib.gtx_sort(self.ctx, _ptr(reads), reads.shape[0], int(n_classes), _ptr(order), _ptr(out)))
        return order, out

    def sort_device(self, d_reads, n_reads, n_classes, d_order, d_sorted=None):
        """raw device addresses; returns when the result is complete"""
        self._chk(self.lib.gtx_sort_device(self.ctx, _ptr(d_reads), int(n_reads), int(n_classes), _ptr(d_order), _ptr(d_sorted)))

    def link(self, regions, values=None, max_difference=0, flags=0):
        """gtx_link: (heads uint32, counts uint32, stops int32, folded values int64 or None, info) of the groups a position-sorted
        stream of (class, start, stop) merges into; values: one int64 per region for LINK_SUM / LINK_MIN / LINK_MAX."""
        regions = _triples(regions)
        n = regions.shape[0]
        v = None if values is None else np.ascontiguousarray(values, dtype=np.int64)
        if v is not None and len(v) != n:
            raise GtxError("link: one value per region")
        heads, counts = np.zeros(max(n, 1), dtype=np.uint32), np.zeros(max(n, 1), dtype=np.uint32)
        stops = np.zeros(max(n, 1), dtype=np.int32)
        folded = None if v is None else np.zeros(max(n, 1), dtype=np.int64)
        info = LinkInfo()
        self._chk(self.lib.gtx_link(self.ctx, _ptr(regions), _ptr(v), n, int(max_difference), int(flags), _ptr(heads), _ptr(counts), _ptr(stops),
                                    _ptr(folded), ctypes.byref(info)))
        g = int(info.n_groups)
        return heads[:g], counts[:g], stops[:g], (None if folded is None or not flags else folded[:g]), info.as_dict()

    def link_device(self, d_regions, n, d_heads, d_counts, d_stops, d_values=None, d_folded=None, max_difference=0, flags=0):
        """gtx_link_device on raw device addresses (outputs sized n); returns the LinkInfo the library fills: read it after sync()."""
        info = LinkInfo()
        self._link_infos = getattr(self, "_link_infos", [])
        self._link_infos.append(info)                       # the library writes it at the next sync: it must live until then
        self._chk(self.lib.gtx_link_device(self.ctx, _ptr(d_regions), _ptr(d_values), int(n), int(max_difference), int(flags), _ptr(d_heads),
                                           _ptr(d_counts), _ptr(d_stops), _ptr(d_folded), ctypes.byref(info)))
        return info

    def adjacent(self, regions, minus=None, op1=0, op2=0, want_dist=False):
        """gtx_adjacent: (distances int64 or None, info) of a position-sorted stream of (class, start, stop): the first region before
        its predecessor, the inclusions and overlaps among same-class neighbours, and with want_dist per region the distance from
        its predecessor's point op1 to its own point op2 (POINTS; INT64_MIN where there is none).  minus: one strand byte per region."""
        regions = _triples(regions)
        n = regions.shape[0]
        m = None if minus is None else np.ascontiguousarray(minus, dtype=np.uint8)
        if m is not None and len(m) != n:
            raise GtxError("adjacent: one strand byte per region")
        dist = np.zeros(n, dtype=np.int64) if want_dist else None
        info = AdjacentInfo()
        self._chk(self.lib.gtx_adjacent(self.ctx, _ptr(regions), _ptr(m), n, int(op1), int(op2), _ptr(dist), ctypes.byref(info)))
        return dist, info.as_dict()

    def adjacent_device(self, d_regions, n, d_minus=None, op1=0, op2=0, d_dist=None):
        """gtx_adjacent_device on raw device addresses; returns the AdjacentInfo the library fills: read it after sync()."""
        info = AdjacentInfo()
        self._link_infos = getattr(self, "_link_infos", [])
        self._link_infos.append(info)                       # the library writes it at the next sync: it must live until then
        self._chk(self.lib.gtx_adjacent_device(self.ctx, _ptr(d_regions), _ptr(d_minus), int(n), int(op1), int(op2), _ptr(d_dist), ctypes.byref(info)))
        return info

    def gaps(self, regions, bounds, capacity=None):
        """gtx_gaps: (owners uint32, starts int32, stops int32, info) of the gaps between the regions of a position-sorted stream inside
        their classes' bounds (int64 per class id, < 0: missing).  When info's n_gaps exceeds `capacity` only the first `capacity`
        gaps are returned; capacity=None grows and repeats the call until everything fits."""
        regions = _triples(regions)
        n = regions.shape[0]
        b = np.ascontiguousarray(bounds, dtype=np.int64)
        info = GapsInfo()
        cap = int(capacity) if capacity is not None else max(1024, n // 4)
        while True:
            owners, starts, stops = np.zeros(max(cap, 1), dtype=np.uint32), np.zeros(max(cap, 1), dtype=np.int32), np.zeros(max(cap, 1), dtype=np.int32)
            self._chk(self.lib.gtx_gaps(self.ctx, _ptr(regions), n, _ptr(b), len(b), cap, _ptr(owners), _ptr(starts), _ptr(stops), ctypes.byref(info)))
            if capacity is not None or info.n_gaps <= cap:
                break
            cap = int(info.n_gaps)
        got = min(int(info.n_gaps), cap)
        return owners[:got], starts[:got], stops[:got], info.as_dict()

    def gaps_device(self, d_regions, n, bounds, capacity, d_owners, d_starts, d_stops):
        """gtx_gaps_device on raw device addresses (bounds: host array; outputs sized capacity); returns the GapsInfo the library
        fills: read it after sync()."""
        b = np.ascontiguousarray(bounds, dtype=np.int64)
        info = GapsInfo()
        self._link_infos = getattr(self, "_link_infos", [])
        self._link_infos.append(info)
        self._chk(self.lib.gtx_gaps_device(self.ctx, _ptr(d_regions), int(n), _ptr(b), len(b), int(capacity), _ptr(d_owners), _ptr(d_starts), _ptr(d_stops),
                                           ctypes.byref(info)))
        return info

    def scan(self, reads, class_len, win_step, win_size, preprocess="1", weights=None, flags=0):
        reads = _triples(reads)
        cl = np.ascontiguousarray(class_len, dtype=np.int32)
        off, tot = scan_layout(cl, win_step, win_size)
        w = None if weights is None else np.ascontiguousarray(weights, dtype=np.int32)
        out = np.zeros(max(tot, 1), dtype=np.uint64)
        self._chk(self.lib.gtx_scan(self.ctx, _ptr(reads), _ptr(w), reads.shape[0], _ptr(cl), len(cl), int(win_step), int(win_size),
                                    preprocess.encode()[0:1], int(flags), _ptr(out), _ptr(off)))
        return out[:tot], off

    def scan_stream(self, pieces, class_len, win_step, win_size, preprocess="1", weighted=False, flags=0, sam=False, fmt=None):
        """gtx_scan_begin .. gtx_scan_end over `pieces`: (reads, weights | None, flags) tuples for packed host batches, or (text bytes,
        TextRules, flags) for blocks of BED text tokenised on the device (sam=True: SAM alignments, GTX_TEXT_SAM; fmt=TEXT_GFF: GFF features).  Returns (windows,
        class offsets, label sum of the text blocks the device took, tickets' needs_host verdicts)."""
        cl = np.ascontiguousarray(class_len, dtype=np.int32)
        off, tot = scan_layout(cl, win_step, win_size)
        out = np.zeros(max(tot, 1), dtype=np.uint64)
        self._chk(self.lib.gtx_scan_begin(self.ctx, _ptr(cl), len(cl), int(win_step), int(win_size), preprocess.encode()[0:1], int(flags), int(weighted), _ptr(off)))
        verdicts = []
        for a, b, fl in pieces:
            if isinstance(a, (bytes, bytearray)):
                t = ctypes.c_int(-1)
                self._chk(self.lib.gtx_scan_add_text(self.ctx, a, len(a), a.count(b"\n"), ctypes.byref(b), int(fl) | _text_format(sam, fmt), ctypes.byref(t)))
                redo = ctypes.c_int(0)
                self._chk(self.lib.gtx_text_result(self.ctx, t.value, ctypes.byref(redo)))
                verdicts.append(redo.value)
            else:
                r = _triples(a)
                w = None if b is None else np.ascontiguousarray(b, dtype=np.int32)
                self._chk(self.lib.gtx_scan_add(self.ctx, _ptr(r), _ptr(w), r.shape[0], int(fl)))
        labels = ctypes.c_int64(0)
        self._chk(self.lib.gtx_scan_end(self.ctx, _ptr(out), ctypes.byref(labels)))
        return out[:tot], off, int(labels.value), verdicts

    def scan_keep(self, slot, reads, class_len, win_step, win_size, preprocess="1", weights=None, flags=0):
        """gtx_scan_begin / gtx_scan_add / gtx_scan_end_keep: the windows of `reads` stay in slot `slot` of the context's HBM.
        Returns (device address, number of windows, class offsets)."""
        reads = _triples(reads)
        cl = np.ascontiguousarray(class_len, dtype=np.int32)
        off, _ = scan_layout(cl, win_step, win_size)
        w = None if weights is None else np.ascontiguousarray(weights, dtype=np.int32)
        self._chk(self.lib.gtx_scan_begin(self.ctx, _ptr(cl), len(cl), int(win_step), int(win_size), preprocess.encode()[0:1], int(flags), int(w is not None), _ptr(off)))
        rc = self.lib.gtx_scan_add(self.ctx, _ptr(reads), _ptr(w), reads.shape[0], int(flags) & READS_UNSORTED)
        if rc != 0:
            self.lib.gtx_scan_end(self.ctx, None, None)            # close the open scan before the error is raised
            self._chk(rc)
        self._chk(self.lib.gtx_scan_end_keep(self.ctx, int(slot), None))
        return self.scan_kept(slot) + (off,)

    def scan_kept(self, slot):
        """(device address, number of windows) of a kept slot"""
        d, n = ctypes.c_void_p(), ctypes.c_int64()
        self._chk(self.lib.gtx_scan_kept(self.ctx, int(slot), ctypes.byref(d), ctypes.byref(n)))
        return int(d.value or 0), int(n.value)

    def scan_kept_read(self, slot):
        """gtx_scan_kept_read: a kept slot's window sums in host memory (uint64, layout of scan); the slot stays as it is"""
        _, n = self.scan_kept(slot)
        out = np.zeros(max(n, 1), dtype=np.uint64)
        self._chk(self.lib.gtx_scan_kept_read(self.ctx, int(slot), _ptr(out)))
        return out[:n]

    def scan_drop(self, slot=-1):
        """free a kept slot (-1: all of them)"""
        self._chk(self.lib.gtx_scan_drop(self.ctx, int(slot)))

    def _kept_or_address(self, v):
        """(device address, number of windows or None) of a window vector given as a kept slot (small int) or a raw device address"""
        if v is None:
            return None, None
        if isinstance(v, (int, np.integer)) and 0 <= int(v) < SCAN_KEEP_SLOTS:
            return self.scan_kept(int(v))
        return int(v), None

    def _grow_and_repeat(self, call, n_windows, capacity, make):
        """A host selector entry with room for `capacity` rows, or, with capacity None, for max(1024, n_windows // 64) rows and then
        for as many as it reported until everything fits.  make(cap) -> (ordinals, rows); call(cap, ordinals, rows, kept) -> rc.
        Returns (ordinals, rows, number kept), the arrays cut to what was written."""
        kept = ctypes.c_int64(0)
        cap = int(capacity) if capacity is not None else max(1024, int(n_windows) // 64)
        while True:
            ordinals, rows = make(max(cap, 1))
            self._chk(call(cap, ordinals, rows, kept))
            if capacity is not None or kept.value <= cap:
                break
            cap = int(kept.value)
        got = min(int(kept.value), cap)
        return ordinals[:got], rows[:got], int(kept.value)

    def window_select(self, tested, tables, window_size, controls=None, n_windows=None, capacity=None, device_out=None):
        """gtx_window_select over window vectors in HBM.  tested / controls: kept slots (small ints, n_windows taken from the slot) or
        raw device addresses (n_windows required); tables: per tested vector its critical counts (window_size + 1 entries with
        controls, one without).  Returns (ordinals int64, rows int32 [kept, columns], number kept); when the number kept exceeds
        `capacity` only the first `capacity` windows are returned.  capacity=None grows and repeats the call until everything fits.
        device_out=(d_ordinals, d_rows): gtx_window_select_device into the caller's device buffers (capacity required), returns the
        number kept."""
        t = [self._kept_or_address(v) for v in tested]
        c = None if controls is None else [self._kept_or_address(v) for v in controls]
        if n_windows is None:
            n_windows = t[0][1]
        nt = len(t)
        d_t = (ctypes.c_void_p * max(nt, 1))(*[a for a, _ in t])
        d_c = None if c is None else (ctypes.c_void_p * max(len(c), 1))(*[a for a, _ in c])
        tabs = [np.ascontiguousarray(x, dtype=np.int32) for x in tables]
        d_k = (ctypes.c_void_p * max(len(tabs), 1))(*[x.ctypes.data for x in tabs])
        cols = nt * (2 if c is not None and any(a for a, _ in c) else 1)
        if device_out is not None:
            kept = ctypes.c_int64(0)
            self._chk(self.lib.gtx_window_select_device(self.ctx, d_t, d_c, nt, int(n_windows), int(window_size), d_k, int(capacity), _ptr(device_out[0]),
                                                        _ptr(device_out[1]), ctypes.byref(kept)))
            return int(kept.value)
        return self._grow_and_repeat(
            lambda cap, ordinals, rows, kept: self.lib.gtx_window_select(self.ctx, d_t, d_c, nt, int(n_windows), int(window_size), d_k, cap, _ptr(ordinals),
                                                                         _ptr(rows), ctypes.byref(kept)),
            n_windows, capacity, lambda cap: (np.full(cap, -1, dtype=np.int64), np.full((cap, max(cols, 1)), -1, dtype=np.int32)))

    def window_refs(self, refs, class_len, class_offsets, win_step, win_size):
        """gtx_window_refs: prepares the regions `refs` ((n, 3) of class, start, stop; any order) on the device for window vectors
        of this geometry (class c at class_offsets[c]): what window_filter tests against until the next call."""
        refs = _triples(np.asarray(refs).reshape(-1, 3))
        cl = np.ascontiguousarray(class_len, dtype=np.int32)
        off = np.ascontiguousarray(class_offsets, dtype=np.int64)
        if len(off) != len(cl):
            raise ValueError("one offset per class")
        self._chk(self.lib.gtx_window_refs(self.ctx, _ptr(refs) if len(refs) else None, len(refs), _ptr(cl), _ptr(off), len(cl), int(win_step), int(win_size)))

    def window_filter(self, windows, min_value=0, n_windows=None, capacity=None, device_out=None):
        """gtx_window_filter over a window vector in HBM: a kept slot (small int, n_windows taken from the slot) or a raw device
        address (n_windows required).  Returns (ordinals int64, values uint64, number kept): the windows with a value >= min_value
        that overlap a region of window_refs, in vector order; when the number kept exceeds `capacity` only the first `capacity`
        are returned.  capacity=None grows and repeats the call until everything fits.  device_out=(d_ordinals, d_values):
        gtx_window_filter_device into the caller's device buffers (capacity required), returns the number kept."""
        addr, n = self._kept_or_address(windows)
        if n_windows is None:
            n_windows = n
        if device_out is not None:
            kept = ctypes.c_int64(0)
            self._chk(self.lib.gtx_window_filter_device(self.ctx, _ptr(addr), int(n_windows), int(min_value), int(capacity), _ptr(device_out[0]),
                                                        _ptr(device_out[1]), ctypes.byref(kept)))
            return int(kept.value)
        return self._grow_and_repeat(
            lambda cap, ordinals, values, kept: self.lib.gtx_window_filter(self.ctx, _ptr(addr), int(n_windows), int(min_value), cap, _ptr(ordinals),
                                                                           _ptr(values), ctypes.byref(kept)),
            n_windows, capacity, lambda cap: (np.full(cap, -1, dtype=np.int64), np.zeros(cap, dtype=np.uint64)))

    def lines_layout(self, block_offset, names, strands, win_step, win_size):
        """gtx_lines_layout: the blocks the line renderer prints by.  block_offset: n_blocks + 1 ordinals ascending from 0; names: one
        str or bytes per block; strands: one '+' or '-' per block.  Returns gtx_lines_max_bytes, the longest line of the layout."""
        off = np.ascontiguousarray(block_offset, dtype=np.int64)
        nm = [x.encode() if isinstance(x, str) else bytes(x) for x in names]
        st = strands.encode() if isinstance(strands, str) else bytes(strands)
        if len(nm) != len(off) - 1 or len(st) != len(nm):
            raise ValueError("one name and one strand per block, one offset more")
        name_off = np.zeros(len(nm) + 1, dtype=np.int32)
        name_off[1:] = np.cumsum([len(x) for x in nm])
        self._chk(self.lib.gtx_lines_layout(self.ctx, _ptr(off), len(nm), b"".join(nm), _ptr(name_off), st, int(win_step), int(win_size)))
        return self.lines_max_bytes()

    def lines_max_bytes(self):
        n = int(self.lib.gtx_lines_max_bytes(self.ctx))
        self._chk(min(n, 0))
        return n

    def set_lines_chunk(self, n_bytes):
        """bytes of bound per range of window_lines / pair_lines (whole tiles; at least one tile)"""
        self._chk(self.lib.gtx_set_lines_chunk(self.ctx, int(n_bytes)))

    def window_lines_device(self, windows, first, count, limit, min_value, d_text, capacity):
        """gtx_window_lines_device: the kept lines of windows [first, first + count) of a kept slot or a raw device address into the
        caller's device buffer.  Returns (lines, bytes, end_at)."""
        addr, _ = self._kept_or_address(windows)
        nl, nb, end = ctypes.c_int64(0), ctypes.c_int64(0), ctypes.c_int64(-1)
        self._chk(self.lib.gtx_window_lines_device(self.ctx, _ptr(addr), int(first), int(count), int(limit), int(min_value), _ptr(d_text), int(capacity),
                                                   ctypes.byref(nl), ctypes.byref(nb), ctypes.byref(end)))
        return int(nl.value), int(nb.value), int(end.value)

    def pair_lines_device(self, d_ordinals, d_values, first, count, limit, d_text, capacity):
        """gtx_pair_lines_device: the same for entries [first, first + count) of (ordinal, value) pairs on the device"""
        nl, nb, end = ctypes.c_int64(0), ctypes.c_int64(0), ctypes.c_int64(-1)
        self._chk(self.lib.gtx_pair_lines_device(self.ctx, _ptr(d_ordinals), _ptr(d_values), int(first), int(count), int(limit), _ptr(d_text), int(capacity),
                                                 ctypes.byref(nl), ctypes.byref(nb), ctypes.byref(end)))
        return int(nl.value), int(nb.value), int(end.value)

    def _lines_stream(self, call, sink):
        """sink(bytes) -> falsy to go on; without one the chunks are collected.  Returns (chunks or None, lines, bytes, end_at)."""
        chunks = []
        take = sink if sink is not None else chunks.append
        cb = LINES_SINK(lambda user, text, n: int(bool(take(ctypes.string_at(text, n)))))
        nl, nb, end = ctypes.c_int64(0), ctypes.c_int64(0), ctypes.c_int64(-1)
        self._chk(call(cb, ctypes.byref(nl), ctypes.byref(nb), ctypes.byref(end)))
        return (chunks if sink is None else None), int(nl.value), int(nb.value), int(end.value)

    def window_lines(self, windows, limit, min_value, n_windows=None, sink=None):
        """gtx_window_lines: all kept lines of a window vector (kept slot, or raw device address with n_windows) streamed in order to
        sink(bytes) (a truthy return ends the call with an error), or collected: returns (list of chunks or None, lines, bytes, end_at)."""
        addr, n = self._kept_or_address(windows)
        if n_windows is None:
            n_windows = n
        return self._lines_stream(lambda cb, nl, nb, end: self.lib.gtx_window_lines(self.ctx, _ptr(addr), int(n_windows), int(limit), int(min_value), cb, None,
                                                                                    nl, nb, end), sink)

    def pair_lines(self, d_ordinals, d_values, n, limit, sink=None):
        """gtx_pair_lines: the same over n (ordinal, value) pairs on the device"""
        return self._lines_stream(lambda cb, nl, nb, end: self.lib.gtx_pair_lines(self.ctx, _ptr(d_ordinals), _ptr(d_values), int(n), int(limit), cb, None,
                                                                                  nl, nb, end), sink)

    def window_filter_lines(self, windows, min_value, limit, n_windows=None, sink=None):
        """gtx_window_filter_lines: window_filter (after window_refs) and pair_lines in one call, the kept windows staying on the device"""
        addr, n = self._kept_or_address(windows)
        if n_windows is None:
            n_windows = n
        return self._lines_stream(lambda cb, nl, nb, end: self.lib.gtx_window_filter_lines(self.ctx, _ptr(addr), int(n_windows), int(min_value), int(limit), cb,
                                                                                           None, nl, nb, end), sink)

    def _peak_vectors(self, signal, control, uniq, n_windows):
        s, c, u = self._kept_or_address(signal), self._kept_or_address(control), self._kept_or_address(uniq)
        if n_windows is None and s[1] is None:
            raise ValueError("n_windows is required when the signal is a raw device address and not a kept slot")
        return s[0], c[0], u[0], (s[1] if n_windows is None else n_windows)

    def peak_select(self, signal, control, win_size, min_reads, uniq=None, norm=False, p_ratio=1.0, n_windows=None, capacity=None):
        """gtx_peak_select over window vectors in HBM: kept slots (small ints, n_windows taken from the signal's slot) or raw device
        addresses (n_windows required); uniq (the mappability track) may be None.  Returns (ordinals int64, rows int64 [kept, 3] of
        v1, v2, v0 after clamp and norm, number kept): the windows with v1 >= min_reads in window order; when the number kept
        exceeds `capacity` only the first `capacity` are returned.  capacity=None grows and repeats the call until everything fits."""
        s, c, u, n_windows = self._peak_vectors(signal, control, uniq, n_windows)
        return self._grow_and_repeat(
            lambda cap, ordinals, rows, kept: self.lib.gtx_peak_select(self.ctx, _ptr(s), _ptr(c), _ptr(u), int(n_windows), int(win_size), int(min_reads),
                                                                       int(bool(norm)), float(p_ratio), cap, _ptr(ordinals), _ptr(rows), ctypes.byref(kept)),
            n_windows, capacity, lambda cap: (np.full(cap, -1, dtype=np.int64), np.full((cap, 3), -1, dtype=np.int64)))

    def peak_select_device(self, signal, control, win_size, min_reads, capacity, d_ordinals, d_rows, uniq=None, norm=False, p_ratio=1.0, n_windows=None):
        """gtx_peak_select_device: the same selection into the caller's device buffers (int64[capacity], int64[capacity * 3]); returns
        the number kept, whatever the capacity."""
        s, c, u, n_windows = self._peak_vectors(signal, control, uniq, n_windows)
        kept = ctypes.c_int64(0)
        self._chk(self.lib.gtx_peak_select_device(self.ctx, _ptr(s), _ptr(c), _ptr(u), int(n_windows), int(win_size), int(min_reads), int(bool(norm)),
                                                  float(p_ratio), int(capacity), _ptr(d_ordinals), _ptr(d_rows), ctypes.byref(kept)))
        return int(kept.value)

    def scan_device(self, d_reads, n_reads, class_len, win_step, win_size, d_out, preprocess="1", d_weights=None, flags=0):
        cl = np.ascontiguousarray(class_len, dtype=np.int32)
        off, tot = scan_layout(cl, win_step, win_size)
        self._chk(self.lib.gtx_scan_device(self.ctx, _ptr(d_reads), _ptr(d_weights), int(n_reads), _ptr(cl), len(cl), int(win_step),
                                           int(win_size), preprocess.encode()[0:1], int(flags), _ptr(d_out), _ptr(off)))
        return off, tot

    def profile(self, on=True):
        """True/1: events around every call; N >= 2: kernel-only events on every N-th call; False/0: off (gtx.h)."""
        self._chk(self.lib.gtx_profile_enable(self.ctx, int(on)))

    def profiled_calls(self):
        return int(self.lib.gtx_profile_count(self.ctx))

    def profile_last(self, back=0):
        """(ms of the streaming kernel, ms of the whole call) of the call `back` calls before the last profiled one."""
        a, b = ctypes.c_float(), ctypes.c_float()
        self._chk(self.lib.gtx_profile_read(self.ctx, int(back), ctypes.byref(a), ctypes.byref(b)))
        return a.value, b.value


def group_plan(ref_class, owner, n_members):
    """(seg_offset[n_members+1], perm[n_refs]) of gtx_group_plan: the compact order of a group's result (pure host code)."""
    rc = np.ascontiguousarray(ref_class, dtype=np.int32)
    ow = np.ascontiguousarray(owner, dtype=np.int32)
    seg = np.zeros(n_members + 1, dtype=np.int64)
    perm = np.zeros(max(len(rc), 1), dtype=np.int32)
    if load().gtx_group_plan(_ptr(rc), 1, len(rc), _ptr(ow), len(ow), int(n_members), _ptr(seg), _ptr(perm)) != 0:
        raise GtxError("gtx_group_plan: bad argument")
    return seg, perm[:len(rc)]


def lpt_assign(class_load, n_members):
    """class -> member by longest-processing-time packing (gtx_lpt_assign: pure host code, no GPU needed)."""
    class_load = np.ascontiguousarray(class_load, dtype=np.int64)
    owner = np.zeros(len(class_load), dtype=np.int32)
    load().gtx_lpt_assign(_ptr(class_load), len(class_load), int(n_members), _ptr(owner))
    return owner


class Group:
    """gtx_group: one context per device, classes dealt to the members, RCCL reduce of the result vector."""

    def __init__(self, devices=None, rank=None, world=None, device=None, unique_id=None):
        """Group(devices): one process drives all members.  Group(rank=r, world=w, device=d, unique_id=bytes): this process holds
        member r of a group of w processes (unique_id from Group.unique_id() on rank 0, handed around by the launcher)."""
        self.lib = load()
        if rank is None:
            ids = np.ascontiguousarray(devices, dtype=np.int32)
            self.g = self.lib.gtx_group_create(len(ids), _ptr(ids))
            self.n, self.n_local, self.rank = len(ids), len(ids), -1
        else:
            buf = None if unique_id is None else ctypes.create_string_buffer(bytes(unique_id), GROUP_ID_BYTES)
            self.g = self.lib.gtx_group_create_rank(int(device), int(rank), int(world), buf)
            self.n, self.n_local, self.rank = int(world), 1, int(rank)
        if not self.g:
            raise GtxError(self.lib.gtx_group_last_error(None).decode())
        self.n_refs = 0

    @staticmethod
    def unique_id():
        """GROUP_ID_BYTES bytes for Group(rank=...) (rank 0 makes it; librccl is loaded for it)."""
        lib = load()
        buf = ctypes.create_string_buffer(GROUP_ID_BYTES)
        if lib.gtx_group_unique_id(buf) != 0:
            raise GtxError(lib.gtx_group_last_error(None).decode())
        return buf.raw

    def ctx(self, member):
        return self.lib.gtx_group_ctx(self.g, int(member))

    def set_stream(self, member, stream_handle):
        c = self.ctx(member)
        if not c:
            raise GtxError("member %d is not local" % member)
        if self.lib.gtx_set_stream(c, ctypes.c_void_p(int(stream_handle))) != 0:
            raise GtxError("gtx_set_stream failed")

    def _ptr_array(self, ptrs):
        return (ctypes.c_void_p * self.n_local)(*[None if p is None else int(p) for p in ptrs])

    def count_device(self, d_reads, n_reads, d_hits, d_weights=None, flags=READS_SORTED):
        """d_reads / n_reads / d_weights: one entry per LOCAL member (raw device addresses); d_hits: n_refs uint64 on member 0's device."""
        # (a loop of calls on the same buffers builds its argument arrays once: a member's call at 1/8 of the reads is ~30 us)
        key = (tuple(d_reads), tuple(n_reads), None if d_weights is None else tuple(d_weights))
        if getattr(self, "_cd_key", None) != key:
            n = np.ascontiguousarray(n_reads, dtype=np.int64)
            self._cd_args = (self._ptr_array(d_reads), None if d_weights is None else self._ptr_array(d_weights), _ptr(n), n)
            self._cd_key = key
        a = self._cd_args
        rc = self.lib.gtx_group_count_device(self.g, a[0], a[1], a[2], flags, d_hits)
        if rc != 0:
            self._chk(rc)

    def scan_device(self, d_reads, n_reads, class_len, win_step, win_size, d_windows, preprocess="1", d_weights=None, flags=0):
        cl = np.ascontiguousarray(class_len, dtype=np.int32)
        off, tot = scan_layout(cl, win_step, win_size)
        n = np.ascontiguousarray(n_reads, dtype=np.int64)
        w = None if d_weights is None else self._ptr_array(d_weights)
        self._chk(self.lib.gtx_group_scan_device(self.g, self._ptr_array(d_reads), w, _ptr(n), _ptr(cl), len(cl), int(win_step), int(win_size),
                                                 preprocess.encode()[0:1], int(flags), _ptr(d_windows), _ptr(off)))
        return off, tot

    def profile(self, member, on=True):
        if self.lib.gtx_profile_enable(self.ctx(member), int(on)) != 0:
            raise GtxError("gtx_profile_enable failed")

    def profiled_calls(self, member):
        return int(self.lib.gtx_profile_count(self.ctx(member)))

    def profile_last(self, member, back=0):
        a, b = ctypes.c_float(), ctypes.c_float()
        if self.lib.gtx_profile_read(self.ctx(member), int(back), ctypes.byref(a), ctypes.byref(b)) != 0:
            raise GtxError("gtx_profile_read failed")
        return a.value, b.value

    def sync(self):
        self._chk(self.lib.gtx_group_sync(self.g))

    def wait_result(self):
        """the members' streams wait (on the device) for the last count_device's exchange"""
        self._chk(self.lib.gtx_group_wait_result(self.g))

    def last_info(self):
        info = CountInfo()
        self._chk(self.lib.gtx_group_last_info(self.g, ctypes.byref(info)))
        return info.as_dict()

    def close(self):
        if getattr(self, "g", None):
            self.lib.gtx_group_destroy(self.g)
            self.g = None

    def __del__(self):
        self.close()

    def _chk(self, rc):
        if rc != 0:
            raise GtxError("gtx group error %d: %s" % (rc, self.lib.gtx_group_last_error(self.g).decode()))

    def assign(self, load):
        load = np.ascontiguousarray(load, dtype=np.int64)
        owner = np.zeros(len(load), dtype=np.int32)
        self._chk(self.lib.gtx_group_assign(self.g, _ptr(load), len(load), _ptr(owner)))
        return owner

    def set_refs(self, refs, n_classes=0, flags=0):
        refs = _triples(refs)
        self._chk(self.lib.gtx_group_set_refs(self.g, _ptr(refs), refs.shape[0], int(n_classes), int(flags)))
        self.n_refs = refs.shape[0]

    def set_ref_blocks(self, first=None, blocks=None):
        if first is None:
            self._chk(self.lib.gtx_group_set_ref_blocks(self.g, None, None))
            return
        first = np.ascontiguousarray(first, dtype=np.int64)
        blocks = np.ascontiguousarray(blocks, dtype=np.int32).reshape(-1, 2)
        self._chk(self.lib.gtx_group_set_ref_blocks(self.g, _ptr(first), _ptr(blocks)))

    def _reduce(self, kind, batches, flags, regions=()):
        begin, add, end = [getattr(self.lib, "gtx_group_%s_%s" % (kind, x)) for x in ("begin", "add", "end")]
        self._chk(begin(self.g))
        for reads, w in batches:
            reads = _triples(reads)
            w = None if w is None else np.ascontiguousarray(w, dtype=np.int32)
            self._chk(add(self.g, _ptr(reads), _ptr(w), reads.shape[0], int(flags)))
        for env, w, first, blocks in regions:
            env = _triples(env)
            w = None if w is None else np.ascontiguousarray(w, dtype=np.int32)
            first = np.ascontiguousarray(first, dtype=np.int64)
            blocks = np.ascontiguousarray(blocks, dtype=np.int32).reshape(-1, 2)
            self._chk(self.lib.gtx_group_count_add_regions(self.g, _ptr(env), _ptr(w), _ptr(first), _ptr(blocks), env.shape[0]))
        out = np.zeros(max(self.n_refs, 1), dtype=np.uint64)
        info = CountInfo()
        self._chk(end(self.g, _ptr(out), ctypes.byref(info)))
        return out[:self.n_refs], info.as_dict()

    def count(self, batches, flags=READS_SORTED, regions=()):
        return self._reduce("count", batches, flags, regions)

    def coverage(self, batches, flags=0):
        return self._reduce("coverage", batches, flags)

    def member_reads(self):
        out = np.zeros(self.n, dtype=np.int64)
        self._chk(self.lib.gtx_group_member_reads(self.g, _ptr(out)))
        return out

    def scan(self, reads, class_len, win_step, win_size, preprocess="1", weights=None, flags=0):
        reads = _triples(reads)
        cl = np.ascontiguousarray(class_len, dtype=np.int32)
        off, tot = scan_layout(cl, win_step, win_size)
        w = None if weights is None else np.ascontiguousarray(weights, dtype=np.int32)
        out = np.zeros(max(tot, 1), dtype=np.uint64)
        self._chk(self.lib.gtx_group_scan(self.g, _ptr(reads), _ptr(w), reads.shape[0], _ptr(cl), len(cl), int(win_step), int(win_size),
                                          preprocess.encode()[0:1], int(flags), _ptr(out), _ptr(off)))
        return out[:tot], off
