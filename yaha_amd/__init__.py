"""yaha_amd -- Python mirror (ctypes) of the C-ABI in include/yaha_hip.h.

The product is the shared library ``yaha_amd/csrc/libyaha_hip.so`` (hand-written HIP kernels for gfx950 plus
the host stages) and the ``yaha`` command line next to it.  This module only loads it and mirrors the
structs; it never falls back to anything else: if the library is missing, importing the bindings raises.
PyTorch is not needed here (bench.py uses it for torch.distributed plumbing only).
"""
import ctypes as C
import os

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.environ.get("YAHA_HIP_LIB", os.path.join(_HERE, "csrc", "libyaha_hip.so"))   # override only for diagnostic builds
CLI_PATH = os.path.join(_HERE, "csrc", "yaha")


class Params(C.Structure):
    _fields_ = [(n, C.c_int32) for n in (
        "wordLen", "maxHits", "bandWidth", "maxGap", "maxIntron", "minMatch", "maxDesert", "minNonOverlap",
        "minRawScore", "minExtLength", "GOCost", "GECost", "RCost", "MScore", "XCutoff")] + [("minIdentity", C.c_float)]


class IndexView(C.Structure):
    _fields_ = [("bases", C.c_void_p), ("n_base_bytes", C.c_uint64), ("maxROff", C.c_uint32),
                ("startingOffs", C.c_void_p), ("ROA", C.c_void_p), ("totalMatches", C.c_uint32), ("wordLen", C.c_int32)]


class ReadBatch(C.Structure):
    _fields_ = [("n_reads", C.c_uint32), ("codes", C.c_void_p), ("offsets", C.c_void_p)]


class Clump(C.Structure):
    _fields_ = [("sro", C.c_uint32), ("sqo", C.c_uint16), ("eqo", C.c_uint16), ("refLen", C.c_uint16),
                ("totScore", C.c_uint16), ("totLength", C.c_uint16), ("matchedBases", C.c_uint16),
                ("mismatchedBases", C.c_uint16), ("gapBases", C.c_uint16), ("status", C.c_uint8),
                ("reserved", C.c_uint8), ("op_start", C.c_uint32), ("n_ops", C.c_uint32)]


COUNTER_NAMES = ("kmer_lookups", "hits", "fragments", "regions", "clumps_formed", "clumps_scored",
                 "dp_ext_calls", "dp_ext_rows", "dp_ext_cells", "dp_gap_calls", "dp_gap_rows", "dp_gap_cells",
                 "perfect_ext_bases", "ref_bases_touched", "ops_out", "splits")


class Counters(C.Structure):
    _fields_ = [(n, C.c_uint64) for n in COUNTER_NAMES]

    def as_dict(self):
        return {n: int(getattr(self, n)) for n in COUNTER_NAMES}


class ResultBatch(C.Structure):
    _fields_ = [("n_reads", C.c_uint32), ("clump_start", C.POINTER(C.c_uint32)), ("clumps", C.POINTER(Clump)),
                ("ops", C.POINTER(C.c_uint32)), ("n_clumps", C.c_uint64), ("n_ops", C.c_uint64), ("counters", Counters)]


class Fragment(C.Structure):
    _fields_ = [("startRefOff", C.c_uint32), ("startQueryOff", C.c_uint16), ("endQueryOff", C.c_uint16),
                ("refLen", C.c_uint16), ("reserved", C.c_uint16), ("read_strand", C.c_uint32)]


class DPProblem(C.Structure):
    _fields_ = [("read", C.c_uint32), ("strand", C.c_uint8), ("mode", C.c_uint8), ("qOff", C.c_uint16),
                ("qLen", C.c_uint16), ("rLen", C.c_uint16), ("rOff", C.c_uint32)]


class DPResult(C.Structure):
    _fields_ = [("score", C.c_int32), ("addedQLen", C.c_uint16), ("addedRLen", C.c_uint16),
                ("op_start", C.c_uint32), ("n_ops", C.c_uint32)]


class PostfilterParams(C.Structure):
    _fields_ = [("minNonOverlap", C.c_int32), ("BPCost", C.c_int32), ("maxBPLog", C.c_int32), ("FBS", C.c_int32), ("FBS_PSLength", C.c_float), ("FBS_PSScore", C.c_float),
                ("bppVmin", C.c_int32), ("bppN", C.c_int32), ("bppThr", C.c_void_p), ("n_seqs", C.c_uint32), ("seq_start", C.c_void_p), ("seq_length", C.c_void_p)]


class DepthParams(C.Structure):
    _fields_ = [("bin", C.c_uint32), ("min_mapq", C.c_uint32), ("n_seqs", C.c_uint32), ("seq_start", C.c_void_p), ("seq_length", C.c_void_p)]


DEPTH_STATS = ("records_counted", "records_skipped_mapq", "records_dropped_two_sequences", "reads_left_to_host")


class EventsParams(C.Structure):
    _fields_ = [("bin", C.c_uint32), ("min_mapq", C.c_uint32), ("min_clip", C.c_uint32), ("n_seqs", C.c_uint32), ("seq_start", C.c_void_p), ("seq_length", C.c_void_p)]


EVENTS_CHANNELS = ("mismatch", "deleted", "insertion", "clip_left", "clip_right")


class PileupParams(C.Structure):
    _fields_ = [("min_mapq", C.c_uint32), ("n_seqs", C.c_uint32), ("seq_start", C.c_void_p), ("seq_length", C.c_void_p)]


PILEUP_CHANNELS = ("A", "C", "G", "T", "N", "del", "ins")
PILEUP_STATS = DEPTH_STATS + ("counts_added",)


class SnvParams(C.Structure):
    """The three costs in 1/100 phred and the three thresholds of a call (include/yaha_hip.h: ygpu_snv_params)."""
    _fields_ = [("cost_match", C.c_uint32), ("cost_error", C.c_uint32), ("cost_het", C.c_uint32), ("min_alt", C.c_uint32), ("min_depth", C.c_uint32),
                ("min_qual", C.c_uint32), ("reserved", C.c_uint32 * 2)]


# one call (ygpu_snv_call, 48 bytes): info = channel of the reference's base | channel of alt << 4 | GT << 8 | the reference's 4-bit code << 12
SNV_CALL_FIELDS = ("slot", "info", "ref_count", "alt_count", "depth", "other", "qual", "gq", "pl0", "pl1", "pl2", "zero")


class IndelParams(C.Structure):
    _fields_ = [("min_mapq", C.c_uint32), ("min_length", C.c_uint32), ("n_seqs", C.c_uint32), ("reserved", C.c_uint32), ("seq_start", C.c_void_p), ("seq_length", C.c_void_p),
                ("capacity", C.c_uint64)]


class IndelEntry(C.Structure):
    """One allele of the device's table: the key's three words (yaha_amd/csrc/indel_core.h) and the records that carry it."""
    _fields_ = [("w0", C.c_uint64), ("w1", C.c_uint64), ("w2", C.c_uint64), ("count", C.c_uint32), ("zero", C.c_uint32)]

    INS_KEPT = 42

    @property
    def slot(self):
        return self.w0 & 0xFFFFFFFF

    @property
    def type(self):
        return "INS" if (self.w0 >> 32) & 1 else "DEL"

    @property
    def length(self):
        return (self.w0 >> 33) & 0xFFFF

    @property
    def bases(self):
        """The kept bases of an insertion as letters (the first 42), '' for a deletion."""
        if self.type == "DEL":
            return ""
        n = min(self.length, self.INS_KEPT)
        return "".join("ACGTN"[min(4, ((self.w1 >> (3 * i)) if i < 21 else (self.w2 >> (3 * (i - 21)))) & 7)] for i in range(n))


class IndelCallParams(C.Structure):
    """The three costs in 1/100 phred and the three thresholds of an indel call (include/yaha_hip.h: ygpu_indelcall_params)."""
    _fields_ = [("cost_match", C.c_uint32), ("cost_error", C.c_uint32), ("cost_het", C.c_uint32), ("min_alt", C.c_uint32), ("min_depth", C.c_uint32),
                ("min_qual", C.c_uint32), ("reserved", C.c_uint32 * 2)]


# one call (ygpu_indel_call, 64 bytes): the normalised key's three words (uint64), then uint32 words; info = GT | the anchor's 4-bit reference code << 4
INDEL_CALL_FIELDS = ("w0", "w1", "w2", "alt_count", "ref_count", "depth", "qual", "gq", "pl0", "pl1", "pl2", "info", "zero")
INDEL_CALL_STATS = ("raw", "shifted", "merged", "skipped")


INDEL_STATS = ("records_counted", "records_skipped_mapq", "records_dropped_two_sequences", "events", "reads_left_to_host", "events_lost")


class EProfileParams(C.Structure):
    _fields_ = [("min_mapq", C.c_uint32), ("n_seqs", C.c_uint32), ("seq_start", C.c_void_p), ("seq_length", C.c_void_p)]


EPROFILE_WORDS = 1556
# the sections of the table (yaha_amd/csrc/eprofile_core.h): name -> (first word, shape)
EPROFILE_SECTIONS = {"SUB": (0, (5, 5)), "INS": (25, (65,)), "DEL": (90, (65,)), "IDENT": (155, (1001,)), "POS": (1156, (100, 4))}


class JunctionParams(C.Structure):
    _fields_ = [("min_mapq", C.c_uint32), ("n_seqs", C.c_uint32), ("seq_start", C.c_void_p), ("seq_length", C.c_void_p)]


class Junction(C.Structure):
    _fields_ = [("read", C.c_uint32), ("ordinal", C.c_uint32), ("seqA", C.c_uint32), ("posA", C.c_uint32), ("seqB", C.c_uint32), ("posB", C.c_uint32),
                ("strandA", C.c_uint8), ("strandB", C.c_uint8), ("type", C.c_uint8), ("reserved", C.c_uint8), ("qgap", C.c_int32)]


JUNCTION_TYPES = ("DEL", "DUP", "INV", "TRA")
JUNCTION_STATS = ("reads_with_junctions", "junctions", "records_skipped_mapq", "reads_left_to_host")


class OutClump(C.Structure):
    _fields_ = [("c", Clump), ("status", C.c_uint8), ("mapQuality", C.c_uint8), ("numSecondaries", C.c_uint16), ("matchedPrimary", C.c_uint16), ("primaryCount", C.c_uint16)]


class FilteredBatch(C.Structure):
    _fields_ = [("n_reads", C.c_uint32), ("clump_start", C.POINTER(C.c_uint32)), ("clumps", C.POINTER(OutClump)), ("ops", C.POINTER(C.c_uint32)),
                ("n_clumps", C.c_uint64), ("n_ops", C.c_uint64), ("counters", Counters)]


class ArenaProfile(C.Structure):
    _fields_ = [("n", C.c_uint32), ("last_clump_slots", C.c_uint32), ("cap", C.c_uint64 * 224), ("trace_ratio", C.c_double), ("ops_ratio", C.c_double), ("last_fall", C.c_int64), ("bases", C.c_uint64)]


DP_FULL, DP_BANDED, DP_EXT_FWD, DP_EXT_REV = 0, 1, 2, 3
DP_KERNELS_AUTO, DP_KERNELS_WAVE, DP_KERNELS_LANES, DP_KERNELS_LANES_CAREFUL = 0, 1, 2, 3

EXPORTS = (
    "ygpu_device_count", "ygpu_init", "ygpu_init_multi", "ygpu_clone", "ygpu_destroy", "ygpu_last_error", "ygpu_memory", "ygpu_park", "ygpu_get_arena_profile", "ygpu_presize", "ygpu_upload", "ygpu_upload_nowait", "ygpu_run", "ygpu_collect", "ygpu_result_size", "ygpu_collect_into", "ygpu_host_alloc", "ygpu_host_free", "ygpu_set_postfilter", "ygpu_postfilter_snapshot", "ygpu_postfilter", "ygpu_postfilter_drop", "ygpu_inject_results", "ygpu_selftest_primitives", "ygpu_trace_volume", "ygpu_filtered_size", "ygpu_collect_filtered", "ygpu_last_timing",
    "ygpu_depth_enable", "ygpu_depth_size", "ygpu_depth_collect", "yaha_session_depth_params",
    "ygpu_events_enable", "ygpu_events_size", "ygpu_events_collect", "yaha_session_events_params",
    "ygpu_pileup_enable", "ygpu_pileup_size", "ygpu_pileup_collect", "ygpu_pileup_candidates_size", "ygpu_pileup_candidates_collect", "ygpu_pileup_gather",
    "yaha_session_pileup_params",
    "ygpu_pileup_add", "ygpu_snv_call_size", "ygpu_snv_collect", "yaha_session_snv_params",
    "ygpu_indels_enable", "ygpu_indels_size", "ygpu_indels_collect", "yaha_session_indel_params",
    "ygpu_indelcall_normalize", "ygpu_indelcall_alleles", "ygpu_indelcall_size", "ygpu_indelcall_collect", "yaha_session_indelcall_params",
    "ygpu_eprofile_enable", "ygpu_eprofile_size", "ygpu_eprofile_collect", "yaha_session_eprofile_params",
    "ygpu_junctions_enable", "ygpu_junctions_size", "ygpu_junctions_collect", "yaha_session_junction_params",
    "ygpu_bgzf_open", "ygpu_bgzf_bound", "ygpu_bgzf_compress", "ygpu_bgzf_last_error", "ygpu_bgzf_close",
    "ygpu_bamsort_open", "ygpu_bamsort_append", "ygpu_bamsort_sort", "ygpu_bamsort_next", "ygpu_bamsort_info", "ygpu_bamsort_last_error", "ygpu_bamsort_close",
    "ygpu_submit", "ygpu_poll", "ygpu_wait", "ygpu_seed_join", "ygpu_seed_join_kept", "ygpu_chain", "ygpu_dp_batch", "ygpu_dp_batch_ex",
    "yaha_session_open", "yaha_session_close", "yaha_session_error", "yaha_session_params",
    "yaha_session_index_view", "yaha_session_header", "yaha_session_next_batch", "yaha_session_emit", "yaha_session_postfilter_params", "yaha_session_emit_filtered",
    "yaha_build_index", "yaha_main")

_lib = None


def lib():
    """Load libyaha_hip.so (fails loudly when it has not been built)."""
    global _lib
    if _lib is None:
        if not os.path.exists(LIB_PATH):
            raise RuntimeError("%s is missing: run `python -c 'import __graft_entry__ as g; g.build()'` "
                               "(or make -C yaha_amd/csrc); there is no fallback path" % LIB_PATH)
        L = C.CDLL(LIB_PATH)
        L.ygpu_last_error.restype = C.c_char_p
        L.yaha_session_error.restype = C.c_char_p
        L.ygpu_bgzf_last_error.restype = C.c_char_p
        L.ygpu_bgzf_last_error.argtypes = [C.c_void_p]
        L.ygpu_bgzf_bound.restype = C.c_uint64
        L.ygpu_bgzf_bound.argtypes = [C.c_uint64]
        L.ygpu_bamsort_last_error.restype = C.c_char_p
        L.ygpu_bamsort_last_error.argtypes = [C.c_void_p]
        L.ygpu_bamsort_info.restype = C.c_uint64
        L.ygpu_bamsort_info.argtypes = [C.c_void_p, C.c_int]
        for name in EXPORTS:
            getattr(L, name)
        _lib = L
    return _lib


def _argv(args):
    arr = (C.c_char_p * len(args))(*[a.encode() if isinstance(a, str) else a for a in args])
    return len(args), arr


def build_index(args):
    """`yaha -g genome.fa [-L k] [-S s] [-H h]` (reference Main.c:554-628)."""
    n, arr = _argv(args)
    rc = lib().yaha_build_index(n, arr)
    if rc != 0:
        raise RuntimeError("yaha_build_index%r failed: %d" % (tuple(args), rc))


class Session:
    """Host stages around the hot path: argument parsing, .nib2/index mapping, read batching, OQC + SAM."""

    def __init__(self, args):
        self._h = C.c_void_p()
        n, arr = _argv(args)
        rc = lib().yaha_session_open(n, arr, C.byref(self._h))
        if rc != 0:
            msg = lib().yaha_session_error(self._h).decode() if self._h else "bad arguments"
            raise RuntimeError("yaha_session_open failed: %d %s" % (rc, msg))
        self.params = Params()
        lib().yaha_session_params(self._h, C.byref(self.params))
        self.index = IndexView()
        lib().yaha_session_index_view(self._h, C.byref(self.index))

    def header(self):
        t, n = C.c_char_p(), C.c_size_t()
        lib().yaha_session_header(self._h, C.byref(t), C.byref(n))
        return C.string_at(t, n.value).decode()

    def next_batch(self, max_reads):
        b = ReadBatch()
        lib().yaha_session_next_batch(self._h, max_reads, C.byref(b))
        return b

    def emit(self, result):
        t, n = C.c_char_p(), C.c_size_t()
        rc = lib().yaha_session_emit(self._h, C.byref(result), C.byref(t), C.byref(n))
        if rc != 0:
            raise RuntimeError("yaha_session_emit failed: %d" % rc)
        return C.string_at(t, n.value).decode()

    def emit_filtered(self, filtered):
        t, n = C.c_char_p(), C.c_size_t()
        rc = lib().yaha_session_emit_filtered(self._h, C.byref(filtered), C.byref(t), C.byref(n))
        if rc != 0:
            raise RuntimeError("yaha_session_emit_filtered failed: %d" % rc)
        return C.string_at(t, n.value).decode()

    def close(self):
        if self._h:
            lib().yaha_session_close(self._h)
            self._h = C.c_void_p()

    def __enter__(self):
        return self

    def __exit__(self, *a):
        self.close()


def device_count():
    """HIP devices visible to this process (ygpu_device_count)."""
    return int(lib().ygpu_device_count())


class Context:
    """One device context = the reference's per-thread QueryState, batched (include/yaha_hip.h)."""

    def __init__(self, index_view, params, device=0, parent=None):
        self._h = C.c_void_p()
        if parent is not None:                      # second context on the parent's device, sharing its index image
            rc = lib().ygpu_clone(parent._h, C.byref(self._h))
        else:
            rc = lib().ygpu_init(device, C.byref(index_view), C.byref(params), C.byref(self._h))
        if rc != 0:
            msg = lib().ygpu_last_error(self._h).decode() if self._h else ""
            raise RuntimeError("ygpu_init failed: %d %s (the HIP path is mandatory; there is no CPU fallback)" % (rc, msg))

    @classmethod
    def on_devices(cls, index_view, params, devices, ctx_per_device=1):
        """Contexts on the listed devices through ygpu_init_multi: the first device takes the index image from the host, every further one from the device before
        it (the same device may be listed twice: two images on one device); ctx_per_device contexts a device share its image.  Returns them device-major."""
        n = len(devices); m = n * ctx_per_device
        devs = (C.c_int * n)(*devices); hs = (C.c_void_p * m)(); rcs = (C.c_int * n)()
        rc = lib().ygpu_init_multi(devs, n, ctx_per_device, C.byref(index_view), C.byref(params), hs, rcs)
        ctxs = []
        for k in range(m):
            c = cls.__new__(cls); c._h = C.c_void_p(hs[k]); ctxs.append(c)
        if rc != 0:
            msgs = ["device %d: %d %s" % (devices[k], rcs[k], lib().ygpu_last_error(ctxs[k * ctx_per_device]._h).decode() if hs[k * ctx_per_device] else "") for k in range(n) if rcs[k]]
            for c in reversed(ctxs):
                c.close()
            raise RuntimeError("ygpu_init_multi failed: %d (%s)" % (rc, "; ".join(msgs)))
        return ctxs

    def _check(self, rc, what):
        if rc != 0:
            raise RuntimeError("%s failed: %d %s" % (what, rc, lib().ygpu_last_error(self._h).decode()))

    def memory(self):
        """(free, total, this context's own) device bytes (ygpu_memory)."""
        f, t, m = C.c_uint64(), C.c_uint64(), C.c_uint64()
        self._check(lib().ygpu_memory(self._h, C.byref(f), C.byref(t), C.byref(m)), "ygpu_memory")
        return int(f.value), int(t.value), int(m.value)

    def selftest_primitives(self, n, seed=1, key_bits=8):
        """The path's own exclusive sums and orderings (device/scan.h), the post-filter's sort on the wave and A2's workgroup sort (device/wgsort.h, both rankings)
        against the host's loops (ygpu_selftest_primitives); raises on a difference."""
        self._check(lib().ygpu_selftest_primitives(self._h, C.c_uint32(n), C.c_uint32(seed), C.c_int(key_bits)), "ygpu_selftest_primitives")

    def arena_profile(self):
        """Capacities of this context's arenas and its batch-to-batch estimates (ygpu_get_arena_profile)."""
        p = ArenaProfile()
        self._check(lib().ygpu_get_arena_profile(self._h, C.byref(p)), "ygpu_get_arena_profile")
        return p

    def presize(self, profile):
        """Give this context the arenas of `profile` in one go (ygpu_presize)."""
        self._check(lib().ygpu_presize(self._h, C.byref(profile)), "ygpu_presize")

    def park(self):
        """Release this context's arenas and its share of the device's memory budget (ygpu_park); it can only be closed afterwards."""
        self._check(lib().ygpu_park(self._h), "ygpu_park")

    def upload(self, batch):
        self._n_reads = int(batch.n_reads)
        self._check(lib().ygpu_upload(self._h, C.byref(batch)), "ygpu_upload")

    def run(self):
        self._check(lib().ygpu_run(self._h), "ygpu_run")

    def collect(self):
        r = ResultBatch()
        self._check(lib().ygpu_collect(self._h, C.byref(r)), "ygpu_collect")
        return r

    def set_postfilter(self, session):
        """The session's OQC / FBS parameters for ygpu_postfilter on this context (raises for runs the device stage does not take)."""
        p = PostfilterParams()
        if lib().yaha_session_postfilter_params(session._h, C.byref(p)) != 0:
            raise RuntimeError("yaha_session_postfilter_params: " + lib().yaha_session_error(session._h).decode())
        self._check(lib().ygpu_set_postfilter(self._h, C.byref(p)), "ygpu_set_postfilter")

    def _enable(self, fill, enable, params, session):
        """enable(context, params) -- a ygpu_*_enable -- with the parameters fill -- the yaha_session_*_params that goes with it -- takes from the session."""
        if fill(session._h, C.byref(params)) != 0:
            raise RuntimeError(fill.__name__ + ": " + lib().yaha_session_error(session._h).decode())
        self._check(enable(self._h, C.byref(params)), enable.__name__)

    def _collect(self, size, collect, make, stat_names):
        """size(context, n) -- a ygpu_*_size --, then collect -- the ygpu_*_collect that goes with it -- into make(n): (the object to return, what the call
        fills); returns (object, n, the statistics as a dict)."""
        n = C.c_uint64()
        self._check(size(self._h, C.byref(n)), size.__name__)
        out, arg = make(n.value); st = (C.c_uint64 * max(4, len(stat_names)))()
        self._check(collect(self._h, arg, st), collect.__name__)
        return out, n.value, {k: int(st[i]) for i, k in enumerate(stat_names)}

    @staticmethod
    def _bins(shape):
        import numpy as np
        a = np.zeros(shape, dtype=np.uint32)
        return a, a.ctypes.data_as(C.POINTER(C.c_uint32))

    def depth_enable(self, session):
        """Read depth of the printed clumps behind postfilter() (ygpu_depth_enable), with the session's -covbin / -covq and sequence table.  After
        set_postfilter(); the contexts of one index image share one array."""
        self._enable(lib().yaha_session_depth_params, lib().ygpu_depth_enable, DepthParams(), session)

    def depth_collect(self):
        """(coverage array of the context's index image as it stands -- one uint32 per bin, a numpy array -- and the statistics as a dict)."""
        bins, n, st = self._collect(lib().ygpu_depth_size, lib().ygpu_depth_collect, lambda n: self._bins(max(1, n)), DEPTH_STATS)
        return bins[:n], st

    def events_enable(self, session):
        """The evidence track of the printed clumps behind postfilter() (ygpu_events_enable), with the session's -evbin / -evq / -evclip and sequence table.
        After set_postfilter(); the contexts of one index image share one array."""
        self._enable(lib().yaha_session_events_params, lib().ygpu_events_enable, EventsParams(), session)

    def events_collect(self):
        """(evidence array of the context's index image as it stands -- numpy uint32 of shape (n_bins, 5), channels EVENTS_CHANNELS -- and the statistics as a dict)."""
        ev, n, st = self._collect(lib().ygpu_events_size, lib().ygpu_events_collect, lambda n: self._bins((max(1, n), len(EVENTS_CHANNELS))), DEPTH_STATS)
        return ev[:n], st

    def pileup_enable(self, session):
        """The allele pileup of the printed clumps behind postfilter() (ygpu_pileup_enable), with the session's -puq and sequence table.  After
        set_postfilter(); the contexts of one index image share one array, 28 bytes a reference base."""
        self._enable(lib().yaha_session_pileup_params, lib().ygpu_pileup_enable, PileupParams(), session)

    def pileup_collect(self):
        """(the whole pileup array of the context's index image as it stands -- numpy uint32 of shape (n_slots, 7), channels PILEUP_CHANNELS -- and the
        statistics as a dict).  For tests and small genomes: pileup_candidates() and pileup_gather() are the way at scale."""
        pu, n, st = self._collect(lib().ygpu_pileup_size, lib().ygpu_pileup_collect, lambda n: self._bins((max(1, n), len(PILEUP_CHANNELS))), PILEUP_STATS)
        return pu[:n], st

    def pileup_candidates(self):
        """The slots of the image's array where at least one read disagrees with the reference, ascending (numpy uint32), selected on the device."""
        import numpy as np
        n = C.c_uint64()
        self._check(lib().ygpu_pileup_candidates_size(self._h, C.byref(n)), "ygpu_pileup_candidates_size")
        out = np.zeros(max(1, n.value), dtype=np.uint32)
        self._check(lib().ygpu_pileup_candidates_collect(self._h, out.ctypes.data_as(C.POINTER(C.c_uint32))), "ygpu_pileup_candidates_collect")
        return out[:n.value]

    def pileup_gather(self, slots):
        """The seven counts of every slot of `slots` (ascending; any integer sequence): numpy uint32 of shape (len(slots), 7)."""
        import numpy as np
        sl = np.ascontiguousarray(slots, dtype=np.uint32); rows = np.zeros((max(1, len(sl)), len(PILEUP_CHANNELS)), dtype=np.uint32)
        self._check(lib().ygpu_pileup_gather(self._h, sl.ctypes.data_as(C.POINTER(C.c_uint32)), C.c_uint64(len(sl)), rows.ctypes.data_as(C.POINTER(C.c_uint32))),
                    "ygpu_pileup_gather")
        return rows[:len(sl)]

    def pileup_add(self, slots, rows):
        """Adds rows[i] (seven counts) to slot slots[i] of the image's array (ygpu_pileup_add): a slot past the array adds nothing, slots may repeat.  The array
        then holds a sum of sources and is no longer the image's own counts."""
        import numpy as np
        sl = np.ascontiguousarray(slots, dtype=np.uint32); rw = np.ascontiguousarray(rows, dtype=np.uint32).reshape(-1, len(PILEUP_CHANNELS))
        if len(sl) != len(rw):
            raise ValueError("pileup_add: %d slots, %d rows" % (len(sl), len(rw)))
        self._check(lib().ygpu_pileup_add(self._h, sl.ctypes.data_as(C.POINTER(C.c_uint32)), rw.ctypes.data_as(C.POINTER(C.c_uint32)), C.c_uint64(len(sl))),
                    "ygpu_pileup_add")

    def snv_calls(self, session_or_params):
        """The SNV calls of the image's array as it stands, ascending by slot, selected and judged on the device (ygpu_snv_call_size / ygpu_snv_collect): a
        structured numpy array with the fields SNV_CALL_FIELDS, all uint32.  The parameters: a SnvParams, or a Session whose options give them."""
        import numpy as np
        p = session_or_params
        if not isinstance(p, SnvParams):
            p = SnvParams()
            if lib().yaha_session_snv_params(session_or_params._h, C.byref(p)) != 0:
                raise RuntimeError("yaha_session_snv_params: " + lib().yaha_session_error(session_or_params._h).decode())
        n = C.c_uint64()
        self._check(lib().ygpu_snv_call_size(self._h, C.byref(p), C.byref(n)), "ygpu_snv_call_size")
        out = np.zeros(max(1, n.value), dtype=np.dtype([(f, np.uint32) for f in SNV_CALL_FIELDS]))
        self._check(lib().ygpu_snv_collect(self._h, out.ctypes.data_as(C.c_void_p)), "ygpu_snv_collect")
        return out[:n.value]

    def indels_enable(self, session, capacity=0):
        """Indel alleles of the printed clumps behind postfilter() (ygpu_indels_enable), counted in a hash table of this context's own, with the session's -idq,
        -idlen and sequence table.  capacity: entries, a power of two; 0: twice the context's batch capacity in bases.  After set_postfilter()."""
        p = IndelParams()
        if lib().yaha_session_indel_params(session._h, C.byref(p)) != 0:
            raise RuntimeError("yaha_session_indel_params: " + lib().yaha_session_error(session._h).decode())
        p.capacity = capacity
        self._check(lib().ygpu_indels_enable(self._h, C.byref(p)), "ygpu_indels_enable")

    def indels_size(self):
        """Entries of the table in use after the last postfilter() (ygpu_indels_size)."""
        n = C.c_uint64()
        self._check(lib().ygpu_indels_size(self._h, C.byref(n)), "ygpu_indels_size")
        return int(n.value)

    def indels_collect(self):
        """(the table's occupied entries in ascending table index -- a list of IndelEntry -- and the statistics since the previous collect as a dict); the
        table is empty afterwards (ygpu_indels_collect)."""
        out, n, st = self._collect(lib().ygpu_indels_size, lib().ygpu_indels_collect, lambda n: ((IndelEntry * max(1, n))(),) * 2, INDEL_STATS)
        return [out[i] for i in range(n)], st

    def indelcall_normalize(self, entries, max_shift=256):
        """Left-normalises and merges raw indel alleles on the device (ygpu_indelcall_normalize; after pileup_enable(), whose layout it uses).  entries: IndelEntry
        objects or (w0, w1, w2, count) tuples.  Returns (merged alleles, the statistics as a dict with the keys INDEL_CALL_STATS)."""
        n = len(entries); arr = (IndelEntry * max(1, n))()
        for i, e in enumerate(entries):
            w0, w1, w2, cnt = (e.w0, e.w1, e.w2, e.count) if isinstance(e, IndelEntry) else e
            arr[i].w0, arr[i].w1, arr[i].w2, arr[i].count, arr[i].zero = w0, w1, w2, cnt, 0
        n_out = C.c_uint64(); st = (C.c_uint64 * 4)()
        self._check(lib().ygpu_indelcall_normalize(self._h, arr, C.c_uint64(n), C.c_uint32(max_shift), C.byref(n_out), st), "ygpu_indelcall_normalize")
        self._ic_n = int(n_out.value)
        return self._ic_n, dict(zip(INDEL_CALL_STATS, (int(x) for x in st)))

    def indelcall_alleles(self):
        """The merged, normalised alleles of the last indelcall_normalize() in the order of the file (ygpu_indelcall_alleles): a list of IndelEntry."""
        n = getattr(self, "_ic_n", 0); out = (IndelEntry * max(1, n))()
        self._check(lib().ygpu_indelcall_alleles(self._h, out), "ygpu_indelcall_alleles")
        return [out[i] for i in range(n)]

    def indel_calls(self, session_or_params):
        """The calls among the merged alleles, judged on the device against the image's pileup array as it stands (ygpu_indelcall_size / ygpu_indelcall_collect): a
        structured numpy array with the fields INDEL_CALL_FIELDS (three uint64, then uint32).  The parameters: an IndelCallParams, or a Session."""
        import numpy as np
        p = session_or_params
        if not isinstance(p, IndelCallParams):
            p = IndelCallParams()
            if lib().yaha_session_indelcall_params(session_or_params._h, C.byref(p)) != 0:
                raise RuntimeError("yaha_session_indelcall_params: " + lib().yaha_session_error(session_or_params._h).decode())
        n = C.c_uint64()
        self._check(lib().ygpu_indelcall_size(self._h, C.byref(p), C.byref(n)), "ygpu_indelcall_size")
        out = np.zeros(max(1, n.value), dtype=np.dtype([(f, np.uint64 if f in ("w0", "w1", "w2") else np.uint32) for f in INDEL_CALL_FIELDS]))
        self._check(lib().ygpu_indelcall_collect(self._h, out.ctypes.data_as(C.c_void_p)), "ygpu_indelcall_collect")
        return out[:n.value]

    def eprofile_enable(self, session):
        """The error profile of the printed clumps behind postfilter() (ygpu_eprofile_enable), in a table of this context's own, with the session's -epq and
        sequence table.  After set_postfilter()."""
        self._enable(lib().yaha_session_eprofile_params, lib().ygpu_eprofile_enable, EProfileParams(), session)

    def eprofile_collect(self):
        """(this context's table as it stands -- numpy uint64 of EPROFILE_WORDS words, sections EPROFILE_SECTIONS -- and the statistics as a dict); nothing is
        cleared (ygpu_eprofile_collect)."""
        import numpy as np

        def make(n):
            a = np.zeros(max(1, n), dtype=np.uint64)
            return a, a.ctypes.data_as(C.POINTER(C.c_uint64))
        words, n, st = self._collect(lib().ygpu_eprofile_size, lib().ygpu_eprofile_collect, make, DEPTH_STATS)
        return words[:n], st

    def junctions_enable(self, session):
        """Split-read junctions of every batch behind postfilter() (ygpu_junctions_enable), with the session's -bpq and sequence table.  After set_postfilter()."""
        self._enable(lib().yaha_session_junction_params, lib().ygpu_junctions_enable, JunctionParams(), session)

    def junctions_collect(self):
        """(the junctions of the batch the last postfilter() filtered, in (read, ordinal) order -- a list of Junction -- and the batch's statistics as a dict)."""
        out, n, st = self._collect(lib().ygpu_junctions_size, lib().ygpu_junctions_collect, lambda n: ((Junction * max(1, n))(),) * 2, JUNCTION_STATS)
        return [out[i] for i in range(n)], st

    def inject_results(self, result):
        """Stage-level test entry: a ResultBatch placed on the device as if ygpu_run had produced it for the uploaded reads."""
        self._check(lib().ygpu_inject_results(self._h, C.byref(result)), "ygpu_inject_results")

    def postfilter_snapshot(self):
        """On the context's thread, after run(): the stage's copy of the batch's results.  The context is then free for the next upload() / run() while
        postfilter() -- on another thread -- works on this one."""
        self._check(lib().ygpu_postfilter_snapshot(self._h), "ygpu_postfilter_snapshot")
        self._snap_reads = self._n_reads

    def postfilter(self):
        """OQC, filter by similarity and mapping quality on the device; returns the clumps that are printed (FilteredBatch; arrays owned by this object).
        Works on the snapshot taken by postfilter_snapshot(), or takes one of the last run()'s results itself."""
        n_reads = getattr(self, "_snap_reads", None)
        if n_reads is None:
            n_reads = self._n_reads
        self._snap_reads = None
        self._check(lib().ygpu_postfilter(self._h), "ygpu_postfilter")
        nc, no = C.c_uint64(), C.c_uint64()
        self._check(lib().ygpu_filtered_size(self._h, C.byref(nc), C.byref(no)), "ygpu_filtered_size")
        self._f_cs = (C.c_uint32 * (n_reads + 1))(); self._f_cl = (OutClump * max(1, nc.value))(); self._f_ops = (C.c_uint32 * max(1, no.value))()
        r = FilteredBatch()
        self._check(lib().ygpu_collect_filtered(self._h, self._f_cs, self._f_cl, self._f_ops, C.byref(r)), "ygpu_collect_filtered")
        return r

    def trace_volume(self):
        """The trace stream of the last run (ygpu_trace_volume): records written by the rows kernel, records a traceback can visit, calls, walkers, bytes a record, arena bytes."""
        v = (C.c_uint64 * 6)()
        self._check(lib().ygpu_trace_volume(self._h, v), "ygpu_trace_volume")
        return {"records_written": v[0], "records_visitable": v[1], "calls": v[2], "walkers": v[3], "record_bytes": v[4], "arena_bytes": v[5]}

    def timing(self):
        tot, n = C.c_float(), C.c_int()
        names, ms = C.POINTER(C.c_char_p)(), C.POINTER(C.c_float)()
        self._check(lib().ygpu_last_timing(self._h, C.byref(tot), C.byref(n), C.byref(names), C.byref(ms)), "ygpu_last_timing")
        return tot.value, {names[i].decode(): ms[i] for i in range(n.value)}

    def seed_join(self, kept=False):
        """The fragments of the uploaded batch (ygpu_seed_join): every one, or with kept=True the array as run() builds it, without the single-hit fragments
        that have no neighbour within maxGap diagonals (ygpu_seed_join_kept)."""
        f, n = C.POINTER(Fragment)(), C.c_uint64()
        call = lib().ygpu_seed_join_kept if kept else lib().ygpu_seed_join
        self._check(call(self._h, C.byref(f), C.byref(n)), call.__name__)
        return f, n.value

    def chain(self):
        f, s, rs, n = C.POINTER(Fragment)(), C.POINTER(C.c_uint32)(), C.POINTER(C.c_uint32)(), C.c_uint64()
        self._check(lib().ygpu_chain(self._h, C.byref(f), C.byref(s), C.byref(rs), C.byref(n)), "ygpu_chain")
        return f, s, rs, n.value

    def dp_batch(self, problems, kernels=DP_KERNELS_AUTO):
        arr = (DPProblem * len(problems))(*problems)
        res, ops, nops = C.POINTER(DPResult)(), C.POINTER(C.c_uint32)(), C.c_uint64()
        self._check(lib().ygpu_dp_batch_ex(self._h, arr, len(problems), kernels, C.byref(res), C.byref(ops), C.byref(nops)), "ygpu_dp_batch_ex")
        return res, ops, nops.value

    def submit(self, batch):
        t = C.c_uint64()
        self._check(lib().ygpu_submit(self._h, C.byref(batch), C.byref(t)), "ygpu_submit")
        return t.value

    def poll(self, ticket):
        return lib().ygpu_poll(self._h, C.c_uint64(ticket))

    def wait(self, ticket):
        r = ResultBatch()
        self._check(lib().ygpu_wait(self._h, C.c_uint64(ticket), C.byref(r)), "ygpu_wait")
        return r

    def close(self):
        if self._h:
            lib().ygpu_destroy(self._h)
            self._h = C.c_void_p()

    def __enter__(self):
        return self

    def __exit__(self, *a):
        self.close()


class Bgzf:
    """BGZF compression on the device (ygpu_bgzf_*): a handle of its own -- stream, device buffers, page-locked staging for inputs of up to max_in_bytes -- that
    touches no Context.  compress(data) returns data's payloads of 65 280 bytes as whole BGZF blocks, one after the other, WITHOUT the end-of-file block (EOF):
    gzip.decompress(b.compress(data) + Bgzf.EOF) == data."""

    EOF = bytes.fromhex("1f8b08040000000000ff0600424302001b0003000000000000000000")
    PAYLOAD_MAX = 65280

    def __init__(self, max_in_bytes, device=0):
        self._h = C.c_void_p()
        rc = lib().ygpu_bgzf_open(device, C.c_uint64(max_in_bytes), C.byref(self._h))
        if rc != 0:
            msg = lib().ygpu_bgzf_last_error(self._h).decode() if self._h else ""
            self.close()
            raise RuntimeError("ygpu_bgzf_open failed: %d %s" % (rc, msg))

    @staticmethod
    def bound(n):
        """Room compress() needs for n input bytes: ceil(n / 65280) * 65536 (ygpu_bgzf_bound)."""
        return int(lib().ygpu_bgzf_bound(n))

    def compress(self, data, out_cap=None):
        data = bytes(data)
        cap = self.bound(len(data)) if out_cap is None else out_cap
        out = C.create_string_buffer(max(1, cap)); n = C.c_uint64()
        rc = lib().ygpu_bgzf_compress(self._h, data, C.c_uint64(len(data)), out, C.c_uint64(cap), C.byref(n))
        if rc != 0:
            raise RuntimeError("ygpu_bgzf_compress failed: %d %s" % (rc, lib().ygpu_bgzf_last_error(self._h).decode()))
        return out.raw[:n.value]

    def close(self):
        if self._h:
            lib().ygpu_bgzf_close(self._h)
            self._h = C.c_void_p()

    def __enter__(self):
        return self

    def __exit__(self, *a):
        self.close()


class BamSortError(RuntimeError):
    """A ygpu_bamsort_* call that failed: .code is the YGPU_E* value, the text carries the handle's message."""

    def __init__(self, what, code, msg):
        RuntimeError.__init__(self, "%s failed: %d %s" % (what, code, msg))
        self.code = code


class BamSort:
    """The coordinate order of BAM records on the device (ygpu_bamsort_*): a handle of its own that touches no Context.  append(bytes, keys, lens) adds a batch
    of whole records (keys: uint64, lens: the records' byte counts, which add up to len(bytes)); sort() orders them -- stable: equal keys keep append order --
    and returns the permutation (numpy uint32: the record number at every sorted place); windows() yields (blocks, n_raw) for every window of window_bytes of
    the sorted stream: whole BGZF blocks without the end-of-file block, and the uncompressed bytes they hold.  segment_bytes / window_bytes 0: the defaults
    (256 MB; 1024 payloads of 65 280 bytes)."""

    PASSES, SEGMENTS, WINDOWS, WINDOW_BYTES, TILE_KEYS, STORE_BYTES, RECORDS = range(7)

    def __init__(self, max_store_bytes, segment_bytes=0, window_bytes=0, device=0):
        self._h = C.c_void_p()
        rc = lib().ygpu_bamsort_open(device, C.c_uint64(max_store_bytes), C.c_uint64(segment_bytes), C.c_uint64(window_bytes), C.byref(self._h))
        if rc != 0:
            msg = lib().ygpu_bamsort_last_error(self._h).decode() if self._h else ""
            self.close()
            raise BamSortError("ygpu_bamsort_open", rc, msg)

    def _check(self, what, rc):
        if rc != 0:
            raise BamSortError(what, rc, lib().ygpu_bamsort_last_error(self._h).decode())

    def info(self, what):
        return int(lib().ygpu_bamsort_info(self._h, what))

    @staticmethod
    def tile_keys():
        """Keys a scatter tile of the radix sort ranks (a workgroup)."""
        return int(lib().ygpu_bamsort_info(None, BamSort.TILE_KEYS))

    @property
    def passes(self):
        return self.info(self.PASSES)

    def append(self, data, keys, lens):
        import numpy as np
        data = bytes(data)
        keys = np.ascontiguousarray(keys, dtype=np.uint64); lens = np.ascontiguousarray(lens, dtype=np.uint32)
        assert len(keys) == len(lens)
        self._check("ygpu_bamsort_append", lib().ygpu_bamsort_append(self._h, data, C.c_uint64(len(data)), keys.ctypes.data_as(C.c_void_p), lens.ctypes.data_as(C.c_void_p),
                                                                     C.c_uint32(len(keys))))

    def sort(self):
        import numpy as np
        perm = np.zeros(self.info(self.RECORDS), dtype=np.uint32)
        self._check("ygpu_bamsort_sort", lib().ygpu_bamsort_sort(self._h, perm.ctypes.data_as(C.c_void_p)))
        return perm

    def next(self):
        """(blocks, n_raw) of the next window; (b"", 0) at the end."""
        cap = int(lib().ygpu_bgzf_bound(self.info(self.WINDOW_BYTES)))
        out = C.create_string_buffer(cap); n = C.c_uint64(); raw = C.c_uint64()
        self._check("ygpu_bamsort_next", lib().ygpu_bamsort_next(self._h, out, C.c_uint64(cap), C.byref(n), C.byref(raw)))
        return out.raw[:n.value], int(raw.value)

    def windows(self):
        while True:
            blocks, n_raw = self.next()
            if not blocks:
                return
            yield blocks, n_raw

    def close(self):
        if self._h:
            lib().ygpu_bamsort_close(self._h)
            self._h = C.c_void_p()

    def __enter__(self):
        return self

    def __exit__(self, *a):
        self.close()


def result_records(r):
    """Flatten a ResultBatch into plain Python tuples (for bit-exact comparisons in tests)."""
    out = []
    for i in range(r.n_reads):
        rec = []
        for k in range(r.clump_start[i], r.clump_start[i + 1]):
            c = r.clumps[k]
            ops = tuple((r.ops[c.op_start + j] & 0xFFFF, chr((r.ops[c.op_start + j] >> 16) & 0xFF)) for j in range(c.n_ops))
            rec.append((c.sro, c.sqo, c.eqo, c.refLen, c.totScore, c.totLength, c.matchedBases, c.mismatchedBases,
                        c.gapBases, c.status, ops))
        out.append(rec)
    return out
