"""ctypes binding of libpfbwt_hip.so (include/pfbwt_hip.h) -- the MI355X engine.

Thin by design: numpy arrays in/out, no algorithmic work here.  The product library is
`pfbwt-f_amd/lib/libpfbwt_hip.so` (hipcc, gfx950).  If it is missing or cannot be loaded this module
raises -- there is no CPU fallback.
"""
import ctypes as C
import os
import numpy as np

_HERE = os.path.dirname(os.path.abspath(__file__))
DEFAULT_LIB = os.path.join(os.path.dirname(_HERE), "lib", "libpfbwt_hip.so")

PFP_OK = 0
FLAG_U64, FLAG_NON_ACGT_TO_A, FLAG_SAI = 1, 2, 4
DA_ROWS, DA_RUNS = 1, 2
LCP_ROWS, LCP_RUNS = 1, 2
DL_INSIDE = 1
E_ARG = -1
E_INVALID_CHAR, E_TOO_LARGE, E_NOMEM, E_HIP, E_ONE_WORD, E_STATE, E_CORRUPT = -2, -3, -4, -5, -6, -7, -8


class PfpError(RuntimeError):
    def __init__(self, status, msg, pos=None, ch=None):
        super().__init__("pfbwt_hip: %s (status %d)" % (msg, status))
        self.status, self.pos, self.ch = status, pos, ch


class ParseSizes(C.Structure):
    _fields_ = [("n", C.c_uint64), ("m", C.c_uint64), ("dwords", C.c_uint64), ("dsize", C.c_uint64)]


class BwtSizes(C.Structure):
    _fields_ = [("nout", C.c_uint64), ("r", C.c_uint64), ("easy_cases", C.c_uint64), ("hard_cases", C.c_uint64)]


class ShardView(C.Structure):
    _fields_ = [("n", C.c_uint64), ("m", C.c_uint64), ("dwords", C.c_uint64), ("dsize", C.c_uint64),
                ("d_dict", C.c_void_p), ("d_ws", C.c_void_p), ("d_pid", C.c_void_p), ("d_ye", C.c_void_p), ("d_last", C.c_void_p),
                ("left_context", C.c_uint64)]

    def nbytes(self, compact=False):
        """byte sizes of the device arrays, in field order (compact: dictionary, word starts, phrase ids -- pfp_merge_shards derives
        the phrase ends and last bytes)"""
        return [self.dsize, 4 * (self.dwords + 1), 4 * self.m] + ([] if compact else [8 * self.m, self.m])


_libs = {}


class ThrInfo(C.Structure):
    _fields_ = [("runs", C.c_uint64), ("none", C.c_uint64), ("long_queries", C.c_uint64), ("max_span", C.c_uint64)]


class MsInfo(C.Structure):
    _fields_ = [(k, C.c_uint64) for k in ("patterns", "bases", "match", "up", "down", "absent", "breaks", "long_breaks", "max_len")]


class RiInfo(C.Structure):
    _fields_ = [(k, C.c_uint64) for k in ("patterns", "bases", "found", "occurrences", "reported", "pieces", "max_count", "max_piece", "phi_steps", "route")]


class MemInfo(C.Structure):
    _fields_ = [(k, C.c_uint64) for k in ("patterns", "bases", "mems", "max_len", "sum_len", "occurrences", "reported", "pieces", "max_count", "max_piece", "phi_steps", "route")]


class DlInfo(C.Structure):
    _fields_ = [(k, C.c_uint64) for k in ("patterns", "bases", "found", "occurrences", "listed", "skipped", "outside", "entries", "max_docs", "chunks", "by_wave", "by_table", "by_sort", "route")]


class MkIndexInfo(C.Structure):
    _fields_ = [(k, C.c_uint64) for k in ("records", "entries", "distinct", "max_list", "rows")]


class MkInfo(C.Structure):
    _fields_ = [(k, C.c_uint64) for k in ("patterns", "bases", "found", "occurrences", "steps", "probes", "capped", "rows", "records", "raw", "listed", "entries", "max_markers", "chunks", "by_wave", "by_sort")]


class LcpInfo(C.Structure):
    _fields_ = [("pairs", C.c_uint64), ("max_lcp", C.c_uint64), ("sum_lcp", C.c_uint64), ("long_pairs", C.c_uint64)]


class IngestInfo(C.Structure):
    _fields_ = [("raw_bytes", C.c_uint64), ("records", C.c_uint64), ("n", C.c_uint64), ("read_wait_ms", C.c_double), ("total_ms", C.c_double), ("mode", C.c_int)]


class PanelInfo(C.Structure):
    _fields_ = [(k, C.c_uint64) for k in ("contigs", "haplotypes", "records", "sites", "kept", "skipped_overlap", "alt_applied", "bases", "min_record", "max_record")]


class VcfInfo(C.Structure):
    _fields_ = [("lines", C.c_uint64), ("samples", C.c_uint64), ("skipped_symbolic", C.c_uint64), ("missing_gt", C.c_uint64), ("panel", PanelInfo)]


class Panel(C.Structure):
    """pfp_panel (include/pfbwt_hip.h)"""
    _fields_ = [("ncontigs", C.c_uint64), ("ref", C.c_void_p), ("ref_off", C.c_void_p), ("contig_names", C.POINTER(C.c_char_p)),
                ("nsites", C.c_uint64), ("site_first", C.c_void_p), ("pos", C.c_void_p), ("span", C.c_void_p), ("allele_first", C.c_void_p),
                ("nalt", C.c_uint64), ("alt_off", C.c_void_p), ("alt_bytes", C.c_void_p),
                ("nhap", C.c_uint64), ("gt", C.c_void_p), ("hap_names", C.POINTER(C.c_char_p))]


PANEL_REF_FIRST, PANEL_RECORDS = 1, 2


def load_library(path=None):
    path = os.path.abspath(path or os.environ.get("PFBWT_HIP_LIB") or DEFAULT_LIB)   # PFBWT_HIP_LIB: another build of the same library
    if path in _libs:
        return _libs[path]
    if not os.path.exists(path):
        raise OSError("HIP library %s not built: run `make -C pfbwt-f_amd` (hipcc --offload-arch=gfx950)" % path)
    L = C.CDLL(path)
    vp, u64, i32 = C.c_void_p, C.c_uint64, C.c_int
    L.pfp_create.restype = vp
    L.pfp_create.argtypes = [i32, u64, C.c_uint, i32, u64, C.POINTER(i32)]
    L.pfp_destroy.argtypes = [vp]
    L.pfp_destroy.restype = None
    L.pfp_strerror.restype = C.c_char_p
    L.pfp_strerror.argtypes = [i32]
    L.pfp_backend.restype = C.c_char_p
    L.pfp_error_detail.argtypes = [vp, C.POINTER(u64), C.POINTER(i32)]
    L.pfp_workspace_needed.restype = u64
    L.pfp_workspace_needed.argtypes = [vp]
    L.pfp_reset.argtypes = [vp]
    L.pfp_parse_feed.argtypes = [vp, vp, u64, i32]
    L.pfp_parse_feed_batch.argtypes = [vp, vp, u64, u64, u64]
    L.pfp_parse_feed_device.argtypes = [vp, vp, u64, i32]
    L.pfp_parse_finalize.argtypes = [vp, C.POINTER(ParseSizes)]
    L.pfp_parse_finalize_shard.argtypes = [vp, C.POINTER(ParseSizes)]
    L.pfp_parse_get.argtypes = [vp, vp, vp, vp, vp, vp]
    L.pfp_parse_bwt.argtypes = [vp]
    L.pfp_parse_bwt_get.argtypes = [vp, vp, vp, vp]
    L.pfp_bwt_load.argtypes = [vp, vp, u64, vp, u64, vp, vp, vp, u64, u64]
    L.pfp_bwt_build.argtypes = [vp, i32, i32, C.POINTER(BwtSizes)]
    L.pfp_parse_feed_device_batch.argtypes = [vp, vp, u64, u64, u64]
    L.pfp_bwt_build_slice.argtypes = [vp, i32, i32, i32, i32, C.POINTER(BwtSizes), C.POINTER(u64), C.POINTER(u64), C.POINTER(u64)]
    L.pfp_bwt_get.argtypes = [vp, vp, vp, vp, vp]
    L.pfp_bwt_device_ptrs.argtypes = [vp, C.POINTER(vp), C.POINTER(vp), C.POINTER(vp), C.POINTER(vp)]
    L.pfp_shard_view_get.argtypes = [vp, C.POINTER(ShardView)]
    L.pfp_parse_feed_left_context.argtypes = [vp]
    L.pfp_shard_load.argtypes = [vp, vp, u64, vp, u64]
    L.pfp_device_copy.argtypes = [vp, vp, vp, u64]
    L.pfp_merge_shards.argtypes = [vp, i32, C.POINTER(ShardView), C.POINTER(ParseSizes)]
    L.pfp_sacak_int_u32.argtypes = [vp, vp, C.c_uint32, C.c_uint32]
    L.pfp_sacak_int_u64.argtypes = [vp, vp, u64, u64]
    L.pfp_marker_array.argtypes = [vp, vp, u64, vp, u64, C.POINTER(u64)]
    L.pfp_marker_array_get.argtypes = [vp, vp]
    L.pfp_gsacak_u32.argtypes = [vp, vp, vp, vp, C.c_uint32]
    L.pfp_gsacak_u64.argtypes = [vp, vp, vp, vp, u64]
    L.pfp_profile_enable.argtypes = [vp, i32]
    L.pfp_profile_reset.argtypes = [vp]
    L.pfp_profile_select.argtypes = [vp, C.c_char_p]
    L.pfp_profile_get.argtypes = [vp, i32, C.POINTER(C.c_char_p), C.POINTER(u64), C.POINTER(C.c_double), C.POINTER(C.c_double)]
    L.pfp_stage_ms.argtypes = [vp, C.POINTER(C.c_double)]
    L.pfp_debug_set.argtypes = [vp, C.c_char_p, C.c_longlong]
    L.pfp_parse_feed_fasta.argtypes = [vp, vp, u64, C.c_uint, C.POINTER(u64)]
    L.pfp_parse_fasta_records.argtypes = [vp, vp, vp]
    L.pfp_parse_reserve.argtypes = [vp, u64]
    L.pfp_parse_feed_fasta_file.argtypes = [vp, C.c_char_p, C.c_uint, C.POINTER(IngestInfo)]
    L.pfp_bwt_build_stream.argtypes = [vp, i32, i32, vp, vp, C.POINTER(BwtSizes)]
    L.pfp_text_length.argtypes = [vp, C.POINTER(u64)]
    L.pfp_bwt_get_expanded.argtypes = [vp, vp, vp, i32]
    L.pfp_text_view.argtypes = [vp, C.POINTER(vp), C.POINTER(u64)]
    if hasattr(L, "pfp_parse_feed_panel"):      # (a library of an earlier commit, loaded for an A/B measurement, has no panel feed)
        L.pfp_parse_feed_panel.argtypes = [vp, C.POINTER(Panel), C.c_uint, C.POINTER(PanelInfo)]
        L.pfp_parse_feed_vcf_file.argtypes = [vp, C.c_char_p, C.c_char_p, C.c_char_p, C.c_uint, C.POINTER(VcfInfo)]
        L.pfp_text_get.argtypes = [vp, u64, u64, vp]
    L.pfp_host_register.argtypes = [vp, u64]
    L.pfp_host_unregister.argtypes = [vp]
    L.pfp_debug_wordsum.argtypes = [vp, vp, u64, C.POINTER(u64)]
    L.pfp_debug_check_sample_order.argtypes = [vp, C.POINTER(u64)]
    L.pfp_debug_check_sa.argtypes = [vp, C.POINTER(u64)]
    L.pfp_parse_feed_device_view.argtypes = [vp, vp, u64, u64, u64]
    L.pfp_debug_check_samples.argtypes = [vp, C.POINTER(u64)]
    if hasattr(L, "pfp_debug_emit_large_groups"):      # (a library of an earlier commit, loaded for an A/B measurement, has no such hook)
        L.pfp_debug_emit_large_groups.argtypes = [vp, C.POINTER(u64)]
    L.pfp_sharded_create.restype = vp
    L.pfp_sharded_create.argtypes = [i32, u64, C.c_uint, i32, C.POINTER(i32), u64, C.POINTER(i32)]
    L.pfp_sharded_destroy.argtypes = [vp]; L.pfp_sharded_destroy.restype = None
    L.pfp_sharded_ctx.restype = vp; L.pfp_sharded_ctx.argtypes = [vp, i32]
    L.pfp_sharded_ranks.argtypes = [vp]
    L.pfp_sharded_build.argtypes = [vp, i32, i32, vp, vp, C.POINTER(u64), C.POINTER(u64), C.POINTER(u64)]
    L.pfp_sharded_reset.argtypes = [vp]
    L.pfp_sharded_error.restype = C.c_char_p; L.pfp_sharded_error.argtypes = [vp]
    L.pfp_parse_docs.argtypes = [vp, C.POINTER(u64)]
    L.pfp_parse_doc_get.argtypes = [vp, u64, C.POINTER(C.c_char_p), C.POINTER(u64)]
    L.pfp_doc_array.argtypes = [vp, vp, u64, C.c_uint]
    L.pfp_doc_array_get.argtypes = [vp, vp, vp, vp]
    L.pfp_doc_array_device_ptrs.argtypes = [vp, C.POINTER(vp), C.POINTER(vp), C.POINTER(vp)]
    L.pfp_doc_array_write.argtypes = [vp, i32, i32, i32]
    L.pfp_lcp_array.argtypes = [vp, C.c_uint, C.POINTER(LcpInfo)]
    L.pfp_lcp_array_get.argtypes = [vp, vp, vp]
    L.pfp_lcp_array_device_ptrs.argtypes = [vp, C.POINTER(vp), C.POINTER(vp)]
    L.pfp_lcp_array_write.argtypes = [vp, i32, i32]
    L.pfp_thresholds.argtypes = [vp, C.POINTER(ThrInfo)]
    L.pfp_thresholds_get.argtypes = [vp, vp, vp]
    L.pfp_thresholds_device_ptrs.argtypes = [vp, C.POINTER(vp), C.POINTER(vp)]
    L.pfp_thresholds_write.argtypes = [vp, i32, i32]
    L.pfp_thresholds_windowed.argtypes = [vp, u64, C.POINTER(ThrInfo), C.POINTER(u64)]
    L.pfp_debug_rows_windowed.argtypes = [vp, u64, vp, vp]
    L.pfp_ms_index.argtypes = [vp]
    L.pfp_ms_query.argtypes = [vp, vp, vp, u64, C.POINTER(MsInfo)]
    L.pfp_ms_query_file.argtypes = [vp, C.c_char_p, C.POINTER(MsInfo)]
    L.pfp_ms_offsets_get.argtypes = [vp, vp, C.POINTER(u64)]
    L.pfp_ms_get.argtypes = [vp, vp, vp]
    L.pfp_ms_device_ptrs.argtypes = [vp, C.POINTER(vp), C.POINTER(vp)]
    L.pfp_ms_write.argtypes = [vp, i32, i32]
    L.pfp_ri_index.argtypes = [vp]
    L.pfp_ri_count.argtypes = [vp, vp, vp, u64, C.POINTER(RiInfo)]
    L.pfp_ri_locate.argtypes = [vp, vp, vp, u64, u64, C.POINTER(RiInfo)]
    L.pfp_ri_query_file.argtypes = [vp, C.c_char_p, i32, u64, C.POINTER(RiInfo)]
    L.pfp_ri_offsets_get.argtypes = [vp, vp, C.POINTER(u64)]
    L.pfp_ri_get.argtypes = [vp, vp, vp]
    L.pfp_ri_device_ptrs.argtypes = [vp, C.POINTER(vp), C.POINTER(vp)]
    L.pfp_ri_write.argtypes = [vp, i32, i32, i32]
    if hasattr(L, "pfp_ri_docs"):                      # (a library of an earlier commit, loaded for an A/B measurement, has no listing)
        L.pfp_ri_docs.argtypes = [vp, vp, vp, u64, vp, u64, C.c_uint, u64, C.POINTER(DlInfo)]
        L.pfp_ri_docs_file.argtypes = [vp, C.c_char_p, vp, u64, C.c_uint, u64, C.POINTER(DlInfo)]
        L.pfp_ri_docs_offsets_get.argtypes = [vp, vp, C.POINTER(u64)]
        L.pfp_ri_docs_get.argtypes = [vp, vp, vp, vp]
        L.pfp_ri_docs_device_ptrs.argtypes = [vp, C.POINTER(vp), C.POINTER(vp), C.POINTER(vp)]
        L.pfp_ri_docs_write.argtypes = [vp, i32, i32, i32, i32]
    if hasattr(L, "pfp_mk_index"):                     # (a library of an earlier commit has no marker queries)
        L.pfp_mk_index.argtypes = [vp, vp, u64, C.POINTER(MkIndexInfo)]
        L.pfp_mk_query.argtypes = [vp, vp, vp, u64, u64, u64, C.POINTER(MkInfo)]
        L.pfp_mk_query_file.argtypes = [vp, C.c_char_p, u64, u64, C.POINTER(MkInfo)]
        L.pfp_mk_offsets_get.argtypes = [vp, vp, C.POINTER(u64)]
        L.pfp_mk_get.argtypes = [vp, vp, vp, vp, vp]
        L.pfp_mk_device_ptrs.argtypes = [vp, C.POINTER(vp), C.POINTER(vp), C.POINTER(vp), C.POINTER(vp)]
        L.pfp_mk_write.argtypes = [vp, i32, i32, i32, i32, i32]
    L.pfp_mem_find.argtypes = [vp, u64, i32, u64, C.POINTER(MemInfo)]
    L.pfp_mem_offsets_get.argtypes = [vp, vp, C.POINTER(u64), vp, C.POINTER(u64)]
    L.pfp_mem_get.argtypes = [vp, vp, vp, vp, vp, vp]
    L.pfp_mem_device_ptrs.argtypes = [vp, C.POINTER(vp), C.POINTER(vp), C.POINTER(vp), C.POINTER(vp), C.POINTER(vp)]
    L.pfp_mem_write.argtypes = [vp, i32, i32, i32, i32, i32]
    _libs[path] = L
    return L


def _ptr(a):
    return None if a is None else a.ctypes.data_as(C.c_void_p)


def _info(inf):
    """the fields of an info structure of 64-bit counters as a dict"""
    return {k: int(getattr(inf, k)) for k, _ in inf._fields_}


class PfpContext:
    """One engine context = one HIP stream + one device workspace (include/pfbwt_hip.h)."""

    def __init__(self, w=10, p=100, u64=True, non_acgt_to_a=False, sai=True, device=0, workspace_bytes=0, lib=None):
        self.L = load_library(lib)
        self.u64 = bool(u64)
        self.udt = np.uint64 if u64 else np.uint32
        flags = (FLAG_U64 if u64 else 0) | (FLAG_NON_ACGT_TO_A if non_acgt_to_a else 0) | (FLAG_SAI if sai else 0)
        self.sai = bool(sai)
        st = C.c_int(0)
        self.h = self.L.pfp_create(int(w), int(p), flags, int(device), int(workspace_bytes), C.byref(st))
        if not self.h:
            raise PfpError(st.value, self.L.pfp_strerror(st.value).decode())
        self.sizes = None
        self.bsizes = None

    def debug_set(self, **switches):
        """route / tuning switches of this context (include/pfbwt_hip_dev.h: pfp_debug_set), e.g. force_wide_rows=1"""
        for k, v in switches.items():
            self._check(self.L.pfp_debug_set(self.h, k.encode(), int(v)))

    def close(self):
        if getattr(self, "h", None):
            if not getattr(self, "_borrowed", False):      # (the contexts of a ShardedBuild belong to its handle)
                self.L.pfp_destroy(self.h)
            self.h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def _check(self, st):
        if st != PFP_OK:
            pos, ch = C.c_uint64(0), C.c_int(0)
            self.L.pfp_error_detail(self.h, C.byref(pos), C.byref(ch))
            raise PfpError(st, self.L.pfp_strerror(st).decode(), pos.value, ch.value)

    def reset(self):
        self._check(self.L.pfp_reset(self.h))

    def _device_ptrs(self, fn, n):
        """what one of the pfp_*_device_ptrs entries answers: n device pointers (None: not made)"""
        p = [C.c_void_p(0) for _ in range(n)]
        self._check(fn(self.h, *[C.byref(x) for x in p]))
        return [x.value for x in p]

    # ---- stage 1
    def feed(self, bases, end_of_seq=True):
        a = np.frombuffer(bases, dtype=np.uint8) if isinstance(bases, (bytes, bytearray, memoryview)) else np.ascontiguousarray(bases, dtype=np.uint8)
        self._check(self.L.pfp_parse_feed(self.h, _ptr(a) if a.size else None, a.size, 1 if end_of_seq else 0))

    def reserve(self, text_bytes):
        self._check(self.L.pfp_parse_reserve(self.h, int(text_bytes)))

    def feed_fasta(self, raw, final=True, records=False, ptr=None, nbytes=None):
        """raw FASTA bytes (bytes / uint8 array, or ptr + nbytes of host memory); returns the (raw offset, text position) pairs of
        the records that start in this call when records=True"""
        if ptr is None:
            a = np.frombuffer(raw, dtype=np.uint8) if isinstance(raw, (bytes, bytearray, memoryview)) else np.ascontiguousarray(raw, dtype=np.uint8)
            ptr, nbytes = a.ctypes.data, a.size
        nrec = C.c_uint64(0)
        self._check(self.L.pfp_parse_feed_fasta(self.h, C.c_void_p(ptr), int(nbytes), (1 if final else 0) | (2 if records else 0), C.byref(nrec)))
        if not records:
            return None
        ro = np.empty(nrec.value, np.uint64); tp = np.empty(nrec.value, np.uint64)
        self._check(self.L.pfp_parse_fasta_records(self.h, _ptr(ro), _ptr(tp)))
        return ro, tp

    def feed_fasta_file(self, path, records=False):
        info = IngestInfo()
        self._check(self.L.pfp_parse_feed_fasta_file(self.h, os.fsencode(path), 2 if records else 0, C.byref(info)))
        return info

    def feed_panel(self, ref, ref_off, site_first, pos, span, allele_first, alt_off, alt_bytes, gt, nhap, ref_first=True, records=False,
                   contig_names=None, hap_names=None, flags=None):
        """the haplotype records of a variant panel, expanded on the device (include/pfbwt_hip.h: pfp_parse_feed_panel).  numpy arrays /
        bytes as the header names them; gt is site-major, nsites * nhap bytes (any shape).  Returns the pfp_panel_info counters."""
        as_u8 = lambda x: np.frombuffer(x, dtype=np.uint8) if isinstance(x, (bytes, bytearray, memoryview)) else np.ascontiguousarray(x, dtype=np.uint8)
        as_u64 = lambda x: None if x is None else np.ascontiguousarray(x, dtype=np.uint64)
        keep = [as_u8(ref), as_u64(ref_off), as_u64(site_first), as_u64(pos), None if span is None else np.ascontiguousarray(span, dtype=np.uint32),
                as_u64(allele_first), as_u64(alt_off), as_u8(alt_bytes), None if gt is None else as_u8(gt).reshape(-1)]
        ptr = lambda a: None if a is None or a.size == 0 else a.ctypes.data
        names = lambda v: None if v is None else (C.c_char_p * len(v))(*[x.encode() if isinstance(x, str) else x for x in v])
        cn, hn = names(contig_names), names(hap_names)
        P = Panel()
        P.ncontigs = 0 if keep[1] is None else max(keep[1].size - 1, 0); P.ref = ptr(keep[0]); P.ref_off = None if keep[1] is None else keep[1].ctypes.data
        P.contig_names = cn
        P.nsites = 0 if keep[3] is None else keep[3].size; P.site_first = None if keep[2] is None else keep[2].ctypes.data
        P.pos, P.span = ptr(keep[3]), ptr(keep[4]); P.allele_first = None if keep[5] is None else keep[5].ctypes.data
        P.nalt = 0 if keep[6] is None else max(keep[6].size - 1, 0); P.alt_off = None if keep[6] is None else keep[6].ctypes.data; P.alt_bytes = ptr(keep[7])
        P.nhap = int(nhap); P.gt = ptr(keep[8]); P.hap_names = hn
        info = PanelInfo()
        fl = ((PANEL_REF_FIRST if ref_first else 0) | (PANEL_RECORDS if records else 0)) if flags is None else int(flags)
        self._check(self.L.pfp_parse_feed_panel(self.h, C.byref(P), fl, C.byref(info)))
        return _info(info)

    def feed_vcf_file(self, ref_fasta, vcf, samples=None, ref_first=True, records=False):
        """reference FASTA + text VCF (plain / gzip) -> one panel feed (pfp_parse_feed_vcf_file); samples: names, a subset in the order
        wanted.  Returns the pfp_vcf_info counters, the panel's under "panel"."""
        info = VcfInfo()
        sm = None if samples is None else (samples if isinstance(samples, str) else ",".join(samples)).encode()
        self._check(self.L.pfp_parse_feed_vcf_file(self.h, os.fsencode(ref_fasta), os.fsencode(vcf), sm, (PANEL_REF_FIRST if ref_first else 0) | (PANEL_RECORDS if records else 0), C.byref(info)))
        return {"lines": int(info.lines), "samples": int(info.samples), "skipped_symbolic": int(info.skipped_symbolic), "missing_gt": int(info.missing_gt), "panel": _info(info.panel)}

    def text_get(self, off=0, length=None):
        """bytes [off, off + length) of the text fed so far, as they are on the device (pfp_text_get)"""
        length = self.text_length() - off if length is None else int(length)
        out = np.empty(length, np.uint8)
        self._check(self.L.pfp_text_get(self.h, int(off), length, _ptr(out)))
        return out.tobytes()

    def docs(self):
        """(name, start) of the records collected by the last file or panel feed (pfp_parse_docs / pfp_parse_doc_get)"""
        n = C.c_uint64(0); self._check(self.L.pfp_parse_docs(self.h, C.byref(n)))
        out = []
        for i in range(n.value):
            nm, st = C.c_char_p(), C.c_uint64(0)
            self._check(self.L.pfp_parse_doc_get(self.h, i, C.byref(nm), C.byref(st)))
            out.append((nm.value.decode(), st.value))
        return out

    def text_length(self):
        n = C.c_uint64(0); self._check(self.L.pfp_text_length(self.h, C.byref(n))); return n.value

    def bwt_build_stream(self, host_bwt_ptr, host_sa_ptr=None, rssa=False):
        """emission with the rows streamed to host memory (n + 1 bytes at host_bwt_ptr, n + 1 U-wide values at host_sa_ptr)"""
        b = BwtSizes()
        self._check(self.L.pfp_bwt_build_stream(self.h, 1 if host_sa_ptr else 0, 1 if rssa else 0, C.c_void_p(host_bwt_ptr), C.c_void_p(host_sa_ptr) if host_sa_ptr else None, C.byref(b)))
        self.bsizes, self._want, self._rows, self.esa_pairs = b, (bool(host_sa_ptr), bool(rssa)), b.nout, b.r
        return b

    def check_sample_order(self):
        """adjacent-row order check of the run samples on the device (include/pfbwt_hip_dev.h)"""
        o = (C.c_uint64 * 5)()
        self._check(self.L.pfp_debug_check_sample_order(self.h, o))
        return {"pairs": int(o[0]), "order_violations": int(o[1]), "rows_not_adjacent": int(o[2]), "max_lcp": int(o[3]), "mean_lcp": (int(o[4]) / int(o[0])) if o[0] else 0.0}

    def check_sa(self):
        """permutation / T[SA-1] == BWT / one EOS byte, checked on the device against the resident text (include/pfbwt_hip_dev.h)"""
        o = (C.c_uint64 * 5)()
        self._check(self.L.pfp_debug_check_sa(self.h, o))
        return {"rows": int(o[0]), "out_of_range": int(o[1]), "duplicates": int(o[2]), "bwt_mismatches": int(o[3]), "eos_bytes": int(o[4])}

    def check_samples(self):
        """the run samples of a -s -r build against its own .bwt / .sa, on the device (include/pfbwt_hip_dev.h)"""
        o = (C.c_uint64 * 3)()
        self._check(self.L.pfp_debug_check_samples(self.h, o))
        return {"runs": int(o[0]), "row_errors": int(o[1]), "value_errors": int(o[2])}

    def emit_large_groups(self):
        """groups that k_emit_groups_large sorted in LDS during the last emission, per list (include/pfbwt_hip_dev.h)"""
        o = (C.c_uint64 * 4)()
        self._check(self.L.pfp_debug_emit_large_groups(self.h, o))
        return {"groups_8k": int(o[0]), "groups_16k": int(o[1]), "rows_8k": int(o[2]), "rows_16k": int(o[3])}

    def bwt_get_expanded(self, host_bwt_ptr, ssa=None, threads=16):
        """.bwt into host memory from its run-length form (one byte per run over PCIe, host threads write the runs)"""
        self._check(self.L.pfp_bwt_get_expanded(self.h, C.c_void_p(host_bwt_ptr), _ptr(ssa), int(threads)))

    def samples_get(self, out=None):
        """the run samples of the last build: (ssa, esa) as 2*r U-wide arrays (into out["ssa"] / out["esa"] if given)"""
        b = self.bsizes
        ssa = out["ssa"] if out else np.empty(2 * b.r, self.udt); esa = out["esa"] if out else np.empty(2 * b.r, self.udt)
        self._check(self.L.pfp_bwt_get(self.h, None, None, _ptr(ssa), _ptr(esa)))
        return ssa, esa

    def feed_host_batch(self, host_ptr, count, length, stride):
        """`count` equal-length records in host memory (pinned: one strided DMA transfer; pageable: staging ring)"""
        self._check(self.L.pfp_parse_feed_batch(self.h, C.c_void_p(int(host_ptr)), int(count), int(length), int(stride)))

    def feed_device_view(self, dptr, count, length, stride):
        """`count` equal-length records in device memory become the text of this parse WITHOUT a copy (they must stay valid until
        finalize returns): pfp_parse_feed_device_view"""
        self._check(self.L.pfp_parse_feed_device_view(self.h, C.c_void_p(int(dptr)), int(count), int(length), int(stride)))

    def feed_device(self, dptr, nbytes, end_of_seq=True):
        self._check(self.L.pfp_parse_feed_device(self.h, C.c_void_p(int(dptr)), int(nbytes), 1 if end_of_seq else 0))

    def finalize(self, shard=False):
        """shard=True: pfp_parse_finalize_shard -- phrases, dictionary words and ids only (a shard that is going to be merged)"""
        s = ParseSizes()
        self._check((self.L.pfp_parse_finalize_shard if shard else self.L.pfp_parse_finalize)(self.h, C.byref(s)))
        self.sizes = s
        return s

    def parse_get(self):
        s = self.sizes
        out = {"dict": np.empty(s.dsize, np.uint8), "occ": np.empty(s.dwords, self.udt), "parse": np.empty(s.m, np.uint32),
               "last": np.empty(s.m, np.uint8), "sai": np.empty(s.m, self.udt) if self.sai else None}
        self._check(self.L.pfp_parse_get(self.h, _ptr(out["dict"]), _ptr(out["occ"]), _ptr(out["parse"]), _ptr(out["last"]), _ptr(out["sai"])))
        return out

    def parse_bwt(self):
        self._check(self.L.pfp_parse_bwt(self.h))

    def parse_bwt_get(self):
        nr = self.sizes.m + 1
        out = {"bwlast": np.empty(nr, np.uint8), "ilist": np.empty(nr, self.udt), "bwsai": np.empty(nr, self.udt) if self.sai else None}
        self._check(self.L.pfp_parse_bwt_get(self.h, _ptr(out["bwlast"]), _ptr(out["ilist"]), _ptr(out["bwsai"])))
        return out

    # ---- multi-GPU sharding
    def feed_device_batch(self, dev_ptr, count, length, stride):
        """`count` equal-length records that already sit in device memory, `stride` bytes apart"""
        self._check(self.L.pfp_parse_feed_device_batch(self.h, C.c_void_p(int(dev_ptr)), int(count), int(length), int(stride)))

    def feed_left_context(self, w=None):
        """shard r > 0: the w 'A's that end the previous shard (pfparser.hpp:335-337); recorded in the shard view"""
        self._check(self.L.pfp_parse_feed_left_context(self.h))

    def shard_load(self, dict_image, parse):
        """a parse saved as .dict / .parse becomes a (stand-alone) shard on the device"""
        d = np.ascontiguousarray(dict_image, np.uint8); p = np.ascontiguousarray(parse, np.uint32)
        self._check(self.L.pfp_shard_load(self.h, _ptr(d), d.size, _ptr(p), p.size))

    def shard_view(self):
        v = ShardView()
        self._check(self.L.pfp_shard_view_get(self.h, C.byref(v)))
        return v

    def device_copy(self, dst_ptr, src_ptr, nbytes):
        self._check(self.L.pfp_device_copy(self.h, C.c_void_p(int(dst_ptr)), C.c_void_p(int(src_ptr)), int(nbytes)))

    def merge_shards(self, views):
        arr = (ShardView * len(views))(*views)
        s = ParseSizes()
        self._check(self.L.pfp_merge_shards(self.h, len(views), arr, C.byref(s)))
        self.sizes = s
        return s

    # ---- stage 2
    def bwt_load(self, dict_, occ, bwlast, ilist, bwsai=None, n_hint=0):
        d = np.ascontiguousarray(dict_, np.uint8); o = np.ascontiguousarray(occ, self.udt)
        bl = np.ascontiguousarray(bwlast, np.uint8); il = np.ascontiguousarray(ilist, self.udt)
        bs = None if bwsai is None else np.ascontiguousarray(bwsai, self.udt)
        if il.size != bl.size or (bs is not None and bs.size != bl.size):      # the ABI takes one row count for the three arrays
            raise PfpError(E_CORRUPT, "bwlast / ilist / bwsai hold different numbers of rows")
        self._check(self.L.pfp_bwt_load(self.h, _ptr(d), d.size, _ptr(o), o.size, _ptr(bl), _ptr(il), _ptr(bs), bl.size, int(n_hint)))

    def bwt_build(self, sa=True, rssa=False):
        b = BwtSizes()
        self._check(self.L.pfp_bwt_build(self.h, 1 if sa else 0, 1 if rssa else 0, C.byref(b)))
        self.bsizes, self._want, self._rows, self.esa_pairs = b, (bool(sa), bool(rssa)), b.nout, b.r
        return b

    def bwt_build_slice(self, slice_index, nslices, sa=True, rssa=False):
        """multi-GPU emission: this context emits only its slice of the output rows; returns (sizes, begin, rows).
        rssa: also the slice's part of the run samples (b.r ssa pairs, self.esa_pairs esa pairs; see include/pfbwt_hip.h)"""
        b = BwtSizes(); beg, rows, ep = C.c_uint64(0), C.c_uint64(0), C.c_uint64(0)
        self._check(self.L.pfp_bwt_build_slice(self.h, 1 if sa else 0, 1 if rssa else 0, int(slice_index), int(nslices), C.byref(b), C.byref(beg), C.byref(rows), C.byref(ep)))
        self.bsizes, self._want, self._rows, self.esa_pairs = b, (bool(sa), bool(rssa)), rows.value, ep.value
        return b, beg.value, rows.value

    def bwt_get(self, out=None):
        """copies the results to host arrays; `out` may hold caller-owned (e.g. page-locked) arrays bwt / sa / ssa / esa that
        are at least as large as needed"""
        b = self.bsizes
        sa, rssa = self._want
        if out is not None:
            need = {"bwt": self._rows, "sa": self._rows if sa else None, "ssa": 2 * b.r if rssa else None, "esa": 2 * getattr(self, "esa_pairs", b.r) if rssa else None}
            for k, cnt in need.items():
                if cnt is not None and (out.get(k) is None or out[k].size < cnt or out[k].dtype != (np.uint8 if k == "bwt" else self.udt)):
                    raise ValueError("bwt_get: out[%r] missing, too small or of the wrong type" % k)
            self._check(self.L.pfp_bwt_get(self.h, _ptr(out["bwt"]), _ptr(out["sa"]) if sa else None, _ptr(out["ssa"]) if rssa else None, _ptr(out["esa"]) if rssa else None))
            return out
        out = {"bwt": np.empty(self._rows, np.uint8), "sa": np.empty(self._rows, self.udt) if sa else None,
               "ssa": np.empty(2 * b.r, self.udt) if rssa else None, "esa": np.empty(2 * getattr(self, "esa_pairs", b.r), self.udt) if rssa else None}
        self._check(self.L.pfp_bwt_get(self.h, _ptr(out["bwt"]), _ptr(out["sa"]), _ptr(out["ssa"]), _ptr(out["esa"])))
        return out

    def bwt_device_ptrs(self):
        return self._device_ptrs(self.L.pfp_bwt_device_ptrs, 4)

    def marker_array(self, mps, sa=None):
        """marker-array post-pass (include/marker_array.hpp:138-174): the .ma stream (uint64 words) for the .mps stream `mps`;
        sa=None: fused with the last bwt_build(sa=True) of this context, else the suffix array given (uint_t values, BWT order)"""
        mps = np.ascontiguousarray(mps, np.uint64)
        n = C.c_uint64(0)
        if sa is None:
            self._check(self.L.pfp_marker_array(self.h, _ptr(mps), mps.size, None, 0, C.byref(n)))
        else:
            sa = np.ascontiguousarray(sa, self.udt)
            self._check(self.L.pfp_marker_array(self.h, _ptr(mps), mps.size, _ptr(sa), sa.size, C.byref(n)))
        out = np.empty(n.value, np.uint64)
        self._check(self.L.pfp_marker_array_get(self.h, _ptr(out) if n.value else None))
        return out

    def doc_array(self, starts, rows=True, runs=True):
        """document arrays of the last build (include/pfbwt_hip.h: pfp_doc_array): `starts` = the record starts b_k (doc_starts,
        or the values of .docs); returns numpy (da, sda, eda) -- None for what was not asked for"""
        st = np.ascontiguousarray(starts, np.uint64)
        self._check(self.L.pfp_doc_array(self.h, _ptr(st), st.size, (DA_ROWS if rows else 0) | (DA_RUNS if runs else 0)))
        b = self.bsizes
        da = np.empty(self._rows, self.udt) if rows else None
        sda = np.empty(2 * b.r, self.udt) if runs else None
        eda = np.empty(2 * getattr(self, "esa_pairs", b.r), self.udt) if runs else None
        self._check(self.L.pfp_doc_array_get(self.h, _ptr(da), _ptr(sda), _ptr(eda)))
        return da, sda, eda

    def doc_array_device_ptrs(self):
        return self._device_ptrs(self.L.pfp_doc_array_device_ptrs, 3)

    def lcp_array(self, rows=True, runs=True):
        """LCP arrays of the last build (include/pfbwt_hip.h: pfp_lcp_array): returns numpy (lcp, slcp, info) -- lcp[i] = LCP[i] for
        every row, slcp = (run-start row, LCP of that row) pairs, None for what was not asked for; info = {"pairs", "max_lcp",
        "sum_lcp", "long_pairs"} of the values at the run starts"""
        inf = LcpInfo()
        self._check(self.L.pfp_lcp_array(self.h, (LCP_ROWS if rows else 0) | (LCP_RUNS if runs else 0), C.byref(inf)))
        lcp = np.empty(self._rows, self.udt) if rows else None
        slcp = np.empty(2 * self.bsizes.r, self.udt) if runs else None
        self._check(self.L.pfp_lcp_array_get(self.h, _ptr(lcp), _ptr(slcp)))
        return lcp, slcp, _info(inf)

    def lcp_array_device_ptrs(self):
        return self._device_ptrs(self.L.pfp_lcp_array_device_ptrs, 2)

    def thresholds(self):
        """Matching-statistics thresholds of the last build (include/pfbwt_hip.h: pfp_thresholds): returns numpy (thr, tlcp, info) --
        thr = (run-start row, threshold row) pairs, tlcp = (run-start row, LCP of the threshold row) pairs, both 0 for a run
        without a threshold; info = {"runs", "none", "long_queries", "max_span"}"""
        inf = ThrInfo()
        self._check(self.L.pfp_thresholds(self.h, C.byref(inf)))
        thr = np.empty(2 * self.bsizes.r, self.udt)
        tlcp = np.empty(2 * self.bsizes.r, self.udt)
        self._check(self.L.pfp_thresholds_get(self.h, _ptr(thr), _ptr(tlcp)))
        return thr, tlcp, _info(inf)

    def thresholds_windowed(self, window_rows=0):
        """The same thresholds without a resident SA (include/pfbwt_hip.h: pfp_thresholds_windowed; needs bwt_build(rssa=True) only):
        the SA is visited in windows of window_rows rows (0: the default, debug_set(thr_window_rows=...)) and the LCP rows come from
        the sparse PLCP.  Returns numpy (thr, tlcp, info, windows) -- the arrays and info of thresholds(), and the windows visited"""
        inf, nwin = ThrInfo(), C.c_uint64(0)
        self._check(self.L.pfp_thresholds_windowed(self.h, int(window_rows), C.byref(inf), C.byref(nwin)))
        thr = np.empty(2 * self.bsizes.r, self.udt)
        tlcp = np.empty(2 * self.bsizes.r, self.udt)
        self._check(self.L.pfp_thresholds_get(self.h, _ptr(thr), _ptr(tlcp)))
        return thr, tlcp, _info(inf), int(nwin.value)

    def debug_rows_windowed(self, window_rows, sa=True, lcp=True):
        """development hook (include/pfbwt_hip_dev.h: pfp_debug_rows_windowed): the SA and LCP rows the windowed thresholds work on,
        window by window to the host; returns numpy (sa, lcp), None for what was not asked for"""
        rows = int(self.bsizes.nout)
        hs = np.empty(rows, self.udt) if sa else None
        hl = np.empty(rows, self.udt) if lcp else None
        self._check(self.L.pfp_debug_rows_windowed(self.h, int(window_rows), _ptr(hs), _ptr(hl)))
        return hs, hl

    def thresholds_device_ptrs(self):
        return self._device_ptrs(self.L.pfp_thresholds_device_ptrs, 2)

    def ms_index(self):
        """Matching-statistics index of the last build (include/pfbwt_hip.h: pfp_ms_index): needs bwt_build(rssa=True) and the
        thresholds of that build (thresholds() or thresholds_windowed()) in this context"""
        self._check(self.L.pfp_ms_index(self.h))

    def ms_query(self, patterns):
        """Matching statistics of a list of byte strings against the indexed build (include/pfbwt_hip.h: pfp_ms_query): returns
        (ptr, len, info) -- two lists with one numpy array per pattern (ptr[j][i] = a text position where the longest prefix of
        patterns[j][i:] that occurs in the text starts, len[j][i] = its length) and info = {"patterns", "bases", "match", "up",
        "down", "absent", "breaks", "long_breaks", "max_len"}"""
        bases, off = self._flat_patterns(patterns)
        ptr, ln, info = self.ms_query_flat(bases, off)
        cut = off[1:-1].astype(np.int64)
        return np.split(ptr, cut) if off.size > 1 else [], np.split(ln, cut) if off.size > 1 else [], info

    def ms_query_flat(self, bases, offsets):
        """the same for patterns given as one byte string (bytes / uint8 array) and len(patterns) + 1 ascending offsets into it;
        returns (ptr, len, info) with offsets[-1] - offsets[0] values per array, the patterns one after the other"""
        a, off = self._pattern_args(bases, offsets)
        inf = MsInfo()
        self._check(self.L.pfp_ms_query(self.h, _ptr(a), _ptr(off), off.size - 1, C.byref(inf)))
        total = int(inf.bases)
        ptr, ln = np.empty(total, self.udt), np.empty(total, self.udt)
        self._check(self.L.pfp_ms_get(self.h, _ptr(ptr), _ptr(ln)))
        return ptr, ln, _info(inf)

    def ms_device_ptrs(self):
        return self._device_ptrs(self.L.pfp_ms_device_ptrs, 2)

    def ri_index(self):
        """Count / locate index of the last build (include/pfbwt_hip.h: pfp_ri_index): needs bwt_build(rssa=True); neither the text
        nor thresholds, so also after bwt_load"""
        self._check(self.L.pfp_ri_index(self.h))

    @staticmethod
    def _flat_patterns(patterns):
        pats = [bytes(x) for x in patterns]
        off = np.zeros(len(pats) + 1, np.uint64)
        if pats:
            off[1:] = np.cumsum([len(x) for x in pats], dtype=np.uint64)
        return b"".join(pats), off

    def _pattern_args(self, bases, offsets):
        a = np.frombuffer(bases, dtype=np.uint8) if isinstance(bases, (bytes, bytearray, memoryview)) else np.ascontiguousarray(bases, dtype=np.uint8)
        off = np.ascontiguousarray(offsets, np.uint64)
        if off.size < 1:
            raise ValueError("offsets holds one more value than there are patterns")
        if a.size == 0:
            a = np.zeros(1, np.uint8)                       # (a non-NULL pointer for patterns that are all empty)
        return a, off

    def ri_count(self, patterns):
        """How often every byte string of a list occurs in the text of the indexed build (include/pfbwt_hip.h: pfp_ri_count):
        returns (cnt, info) -- one count per pattern and info = {"patterns", "bases", "found", "occurrences", ...}"""
        return self.ri_count_flat(*self._flat_patterns(patterns))

    def ri_count_flat(self, bases, offsets):
        a, off = self._pattern_args(bases, offsets)
        inf = RiInfo()
        self._check(self.L.pfp_ri_count(self.h, _ptr(a), _ptr(off), off.size - 1, C.byref(inf)))
        cnt = np.empty(off.size - 1, self.udt)
        self._check(self.L.pfp_ri_get(self.h, _ptr(cnt) if cnt.size else None, None))
        return cnt, _info(inf)

    def ri_locate(self, patterns, max_occ=0):
        """Where every byte string of a list occurs (include/pfbwt_hip.h: pfp_ri_locate): returns (pos, cnt, info) -- pos: one numpy
        array per pattern with the text positions of its occurrences in suffix order (all of them, or with max_occ > 0 those of the last
        min(cnt, max_occ) rows of its interval), cnt: the true counts"""
        bases, off = self._flat_patterns(patterns)
        pos, ooff, cnt, info = self.ri_locate_flat(bases, off, max_occ)
        return (np.split(pos, ooff[1:-1].astype(np.int64)) if cnt.size else []), cnt, info

    def ri_locate_flat(self, bases, offsets, max_occ=0):
        """the same for patterns given as one byte string and len(patterns) + 1 ascending offsets into it; returns (pos, pos_offsets,
        cnt, info): pattern j owns pos[pos_offsets[j] : pos_offsets[j + 1]] (64-bit offsets)"""
        a, off = self._pattern_args(bases, offsets)
        inf = RiInfo()
        self._check(self.L.pfp_ri_locate(self.h, _ptr(a), _ptr(off), off.size - 1, int(max_occ), C.byref(inf)))
        cnt, pos, ooff = np.empty(off.size - 1, self.udt), np.empty(int(inf.reported), self.udt), np.empty(off.size, np.uint64)
        self._check(self.L.pfp_ri_offsets_get(self.h, _ptr(ooff), None))
        self._check(self.L.pfp_ri_get(self.h, _ptr(cnt) if cnt.size else None, _ptr(pos) if pos.size else None))
        return pos, ooff, cnt, _info(inf)

    def ri_device_ptrs(self):
        return self._device_ptrs(self.L.pfp_ri_device_ptrs, 2)

    def ri_docs(self, patterns, starts, inside=False, max_count=0):
        """In which documents every byte string of a list occurs and how often in each (include/pfbwt_hip.h: pfp_ri_docs): `starts` =
        the record starts (doc_starts, the values of .docs, or a coarser table).  Returns (cnt, docs, freqs, info) -- cnt: the true
        counts; docs / freqs: one numpy array per pattern with the documents, ascending, and the occurrences in each.  inside: only
        occurrences that lie inside their record without touching the pad count; max_count > 0: a pattern that occurs more often is
        skipped (no pairs).  info = {"patterns", "bases", "found", "occurrences", "listed", "skipped", "outside", "entries", ...}"""
        bases, off = self._flat_patterns(patterns)
        cnt, doff, doc, freq, info = self.ri_docs_flat(bases, off, starts, inside, max_count)
        cut = doff[1:-1].astype(np.int64)
        return cnt, (np.split(doc, cut) if cnt.size else []), (np.split(freq, cut) if cnt.size else []), info

    def ri_docs_flat(self, bases, offsets, starts, inside=False, max_count=0):
        """the same for patterns given as one byte string and len(patterns) + 1 ascending offsets into it; returns (cnt, doc_offsets,
        doc, freq, info): pattern j owns doc / freq[doc_offsets[j] : doc_offsets[j + 1]] (64-bit offsets)"""
        a, off = self._pattern_args(bases, offsets)
        st = np.ascontiguousarray(starts, np.uint64)
        inf = DlInfo()
        self._check(self.L.pfp_ri_docs(self.h, _ptr(a), _ptr(off), off.size - 1, _ptr(st) if st.size else None, st.size, DL_INSIDE if inside else 0, int(max_count), C.byref(inf)))
        cnt, doff = np.empty(off.size - 1, self.udt), np.empty(off.size, np.uint64)
        doc, freq = np.empty(int(inf.entries), self.udt), np.empty(int(inf.entries), self.udt)
        self._check(self.L.pfp_ri_docs_offsets_get(self.h, _ptr(doff), None))
        self._check(self.L.pfp_ri_docs_get(self.h, _ptr(cnt) if cnt.size else None, _ptr(doc) if doc.size else None, _ptr(freq) if freq.size else None))
        return cnt, doff, doc, freq, _info(inf)

    def ri_docs_device_ptrs(self):
        """device pointers of cnt, doc, freq of the last ri_docs (None: not made)"""
        return self._device_ptrs(self.L.pfp_ri_docs_device_ptrs, 3)

    def mk_index(self, ma=None):
        """Marker index of the last build (include/pfbwt_hip.h: pfp_mk_index): ma=None takes the stream the last fused marker_array of
        this build left on the device, else the .ma stream given (uint64 words).  Returns info = {"records", "entries", "distinct",
        "max_list", "rows"}"""
        inf = MkIndexInfo()
        if ma is None:
            self._check(self.L.pfp_mk_index(self.h, None, 0, C.byref(inf)))
        else:
            ma = np.ascontiguousarray(ma, np.uint64)
            self._check(self.L.pfp_mk_index(self.h, _ptr(ma) if ma.size else _ptr(np.zeros(1, np.uint64)), ma.size, C.byref(inf)))
        return _info(inf)

    def mk_query(self, patterns, min_len=0, max_rows=0):
        """Which markers the occurrences of every byte string of a list overlap, and in how many rows each (include/pfbwt_hip.h:
        pfp_mk_query).  min_len=0: the whole pattern only; min_len=L: every suffix of at least L bytes; max_rows > 0: a suffix with more
        occurrences contributes nothing.  Returns (cnt, probes, markers, freqs, info) -- cnt: the true counts of the whole patterns;
        probes: the probed suffixes; markers / freqs: one uint64 numpy array per pattern, the marker values ascending"""
        bases, off = self._flat_patterns(patterns)
        cnt, probes, moff, marker, freq, info = self.mk_query_flat(bases, off, min_len, max_rows)
        cut = moff[1:-1].astype(np.int64)
        return cnt, probes, (np.split(marker, cut) if cnt.size else []), (np.split(freq, cut) if cnt.size else []), info

    def mk_query_flat(self, bases, offsets, min_len=0, max_rows=0):
        """the same for patterns given as one byte string and len(patterns) + 1 ascending offsets into it; returns (cnt, probes,
        mk_offsets, marker, freq, info): pattern j owns marker / freq[mk_offsets[j] : mk_offsets[j + 1]] (64-bit offsets and values)"""
        a, off = self._pattern_args(bases, offsets)
        inf = MkInfo()
        self._check(self.L.pfp_mk_query(self.h, _ptr(a), _ptr(off), off.size - 1, int(min_len), int(max_rows), C.byref(inf)))
        cnt, probes, moff = np.empty(off.size - 1, self.udt), np.empty(off.size - 1, self.udt), np.empty(off.size, np.uint64)
        marker, freq = np.empty(int(inf.entries), np.uint64), np.empty(int(inf.entries), np.uint64)
        self._check(self.L.pfp_mk_offsets_get(self.h, _ptr(moff), None))
        self._check(self.L.pfp_mk_get(self.h, _ptr(cnt) if cnt.size else None, _ptr(probes) if probes.size else None, _ptr(marker) if marker.size else None, _ptr(freq) if freq.size else None))
        return cnt, probes, moff, marker, freq, _info(inf)

    def mk_device_ptrs(self):
        """device pointers of cnt, probes, marker, freq of the last mk_query (None: not made)"""
        return self._device_ptrs(self.L.pfp_mk_device_ptrs, 4)

    def mem_find(self, min_len=1, locate=False, max_occ=0):
        """Maximal exact matches of the patterns of the last ms_query against the indexed build (include/pfbwt_hip.h: pfp_mem_find):
        returns (start, len, ptr, info) -- three lists with one numpy array per pattern: where every MEM of at least min_len bases
        starts in the pattern, its length and a text position where it occurs -- or, with locate (needs ri_index()), (start, len, ptr,
        cnt, pos, info): cnt one array per pattern with the number of occurrences of each of its MEMs, pos one array per MEM, all
        patterns' MEMs one after the other, with the text positions of its occurrences in suffix order (all, or with max_occ > 0 those
        of the last min(cnt, max_occ) rows of its interval).  info = {"patterns", "bases", "mems", "max_len", "sum_len", "occurrences",
        "reported", "pieces", "max_count", "max_piece", "phi_steps", "route"}"""
        f = self.mem_find_flat(min_len, locate, max_occ)
        cut = f["mem_off"][1:-1].astype(np.int64)
        per = lambda a: np.split(a, cut) if f["mem_off"].size > 1 else []
        out = (per(f["start"]), per(f["len"]), per(f["ptr"]))
        if locate:
            out += (per(f["cnt"]), np.split(f["pos"], f["pos_off"][1:-1].astype(np.int64)) if f["cnt"].size else [])
        return out + (f["info"],)

    def mem_find_flat(self, min_len=1, locate=False, max_occ=0):
        """the same as flat arrays: a dict with start, len, ptr (one value per MEM), mem_off (patterns + 1 64-bit values: the MEMs in
        front of every pattern), info, and with locate cnt, pos and pos_off (MEMs + 1 64-bit offsets into pos)"""
        inf = MemInfo()
        self._check(self.L.pfp_mem_find(self.h, int(min_len), 1 if locate else 0, int(max_occ), C.byref(inf)))
        mems = int(inf.mems)
        out = {k: np.empty(mems, self.udt) for k in ("start", "len", "ptr")}
        out["mem_off"] = np.empty(int(inf.patterns) + 1, np.uint64)
        if locate:
            out["cnt"], out["pos"], out["pos_off"] = np.empty(mems, self.udt), np.empty(int(inf.reported), self.udt), np.empty(mems + 1, np.uint64)
        self._check(self.L.pfp_mem_offsets_get(self.h, _ptr(out["mem_off"]), None, _ptr(out.get("pos_off")), None))
        arg = lambda k: _ptr(out[k]) if k in out and out[k].size else None
        self._check(self.L.pfp_mem_get(self.h, arg("start"), arg("len"), arg("ptr"), arg("cnt"), arg("pos")))
        out["info"] = _info(inf)
        return out

    def mem_device_ptrs(self):
        """device pointers of start, len, ptr, cnt, pos of the last mem_find (None: not made)"""
        return self._device_ptrs(self.L.pfp_mem_device_ptrs, 5)

    # ---- instrumentation
    def profile_enable(self, on=True):
        self._check(self.L.pfp_profile_enable(self.h, 1 if on else 0))

    def profile_select(self, kernel):
        self._check(self.L.pfp_profile_select(self.h, kernel.encode()))

    def profile_reset(self):
        self._check(self.L.pfp_profile_reset(self.h))

    def profile(self):
        rows, i = [], 0
        while True:
            name, n, ms, by = C.c_char_p(), C.c_uint64(), C.c_double(), C.c_double()
            if self.L.pfp_profile_get(self.h, i, C.byref(name), C.byref(n), C.byref(ms), C.byref(by)) != PFP_OK:
                break
            if n.value:
                rows.append({"kernel": name.value.decode(), "launches": n.value, "ms": ms.value, "bytes": by.value})
            i += 1
        return rows

    def stage_ms(self):
        a = (C.c_double * 3)()
        self._check(self.L.pfp_stage_ms(self.h, a))
        return {"parse_finalize": a[0], "parse_bwt": a[1], "bwt_build": a[2]}

    def backend(self):
        return self.L.pfp_backend().decode()


class ShardedBuild:
    """N devices driven from one process (include/pfbwt_hip.h: pfp_sharded_*): rank r's run of whole sequences is fed into
    self.rank(r) (a PfpContext view of the library-owned context), build() makes every rank parse, exchange (RCCL between distinct
    devices), merge, sort and emit its slice; self.rank(r).bwt_get() then returns slice r."""

    def __init__(self, ndev, devices=None, w=10, p=100, u64=True, non_acgt_to_a=False, sai=True, workspace_bytes=0, lib=None):
        self.L = load_library(lib)
        flags = (FLAG_U64 if u64 else 0) | (FLAG_NON_ACGT_TO_A if non_acgt_to_a else 0) | (FLAG_SAI if sai else 0)
        st = C.c_int(0)
        dv = (C.c_int * ndev)(*devices) if devices is not None else None
        self.h = self.L.pfp_sharded_create(int(w), int(p), flags, int(ndev), dv, int(workspace_bytes), C.byref(st))
        if not self.h:
            raise PfpError(st.value, self.L.pfp_strerror(st.value).decode())
        self.ndev = ndev
        self._ranks = []
        for r in range(ndev):      # views of the library-owned contexts (closing them is the sharded handle's business)
            c = PfpContext.__new__(PfpContext)
            c.L, c.u64, c.udt, c.sai, c.sizes, c.bsizes = self.L, bool(u64), (np.uint64 if u64 else np.uint32), bool(sai), None, None
            c.h = self.L.pfp_sharded_ctx(self.h, r); c._borrowed = True
            self._ranks.append(c)

    def rank(self, r):
        return self._ranks[r]

    def build(self, sa=True, rssa=False):
        """returns (parse sizes of the whole collection, [(BwtSizes, first row, rows) per rank])"""
        n = self.ndev
        ps = ParseSizes(); bs = (BwtSizes * n)(); beg = (C.c_uint64 * n)(); rows = (C.c_uint64 * n)(); ep = (C.c_uint64 * n)()
        st = self.L.pfp_sharded_build(self.h, 1 if sa else 0, 1 if rssa else 0, C.byref(ps), bs, beg, rows, ep)
        if st != PFP_OK:
            raise PfpError(st, self.L.pfp_strerror(st).decode() + " [" + self.L.pfp_sharded_error(self.h).decode() + "]")
        out = []
        for r, c in enumerate(self._ranks):
            b = BwtSizes(); C.memmove(C.byref(b), C.byref(bs[r]), C.sizeof(BwtSizes))
            c.bsizes, c._want, c._rows, c.esa_pairs = b, (bool(sa), bool(rssa)), int(rows[r]), int(ep[r])
            out.append((b, int(beg[r]), int(rows[r])))
        return ps, out

    def reset(self):
        st = self.L.pfp_sharded_reset(self.h)
        if st != PFP_OK:
            raise PfpError(st, self.L.pfp_strerror(st).decode())

    def close(self):
        if getattr(self, "h", None):
            for c in self._ranks:
                c.h = None
            self.L.pfp_sharded_destroy(self.h); self.h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


def doc_starts(lengths, w):
    """record starts b_k of records of the given lengths, each followed by its w 'A's: b_0 = 0, b_{k+1} = b_k + len_k + w (what
    .docs holds) -- the table of PfpContext.doc_array for texts fed with feed / feed_device_batch / feed_device_view.  A device batch
    of `count` records of `len` bases: doc_starts([len] * count, w), i.e. k * (len + w)."""
    ln = np.asarray(lengths, np.uint64).reshape(-1)
    out = np.zeros(ln.size, np.uint64)
    if ln.size > 1:
        np.cumsum(ln[:-1] + np.uint64(w), out=out[1:])
    return out


def sacak_int(s, k, u64=False, lib=None):
    """Drop-in for sacak_int (gsa/gsacak.h:88): suffix array of an integer string ending in a unique 0."""
    L = load_library(lib)
    s = np.ascontiguousarray(s, np.uint32)
    SA = np.empty(s.size, np.uint64 if u64 else np.uint32)
    fn = L.pfp_sacak_int_u64 if u64 else L.pfp_sacak_int_u32
    r = fn(_ptr(s), _ptr(SA), s.size, int(k))
    if r < 0:
        raise PfpError(r, "sacak_int failed")
    return SA, r


def gsacak(s, lcp=False, da=False, u64=False, lib=None):
    """Drop-in for gsacak (gsa/gsacak.h:86-96) on a dictionary image: returns (SA, LCP or None, DA or None, rounds)."""
    L = load_library(lib)
    s = np.ascontiguousarray(s, np.uint8)
    ut, it = (np.uint64, np.int64) if u64 else (np.uint32, np.int32)
    SA = np.empty(s.size, ut); LCP = np.empty(s.size, it) if lcp else None; DA = np.empty(s.size, it) if da else None
    r = (L.pfp_gsacak_u64 if u64 else L.pfp_gsacak_u32)(_ptr(s), _ptr(SA), _ptr(LCP), _ptr(DA), s.size)
    if r < 0:
        raise PfpError(r, "gsacak failed")
    return SA, LCP, DA, r
