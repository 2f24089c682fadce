"""ctypes binding of libmdx.so (include/mdx.h) — the product path.

There is no CPU fallback here: if the HIP library is missing or no GPU is visible the
constructor raises.  ``DamageEngine`` replaces the three accumulator objects the reference
creates in mapdamage/main.py:147-155 and the loop body main.py:165-217 that feeds them.
"""

import ctypes
import os
import pathlib

import numpy as np

from . import layout as L
from .batch import ReadBatch, Reference
from .tables import TableSet

_HERE = pathlib.Path(__file__).resolve().parent
_LIBPATH = _HERE / "libmdx.so"
_lib = None

EXPORTS = (
    "mdx_abi_version", "mdx_strerror", "mdx_create", "mdx_destroy", "mdx_last_error",
    "mdx_set_stream", "mdx_set_reference", "mdx_batch_upload", "mdx_batch_free",
    "mdx_tabulate_host", "mdx_tabulate_device", "mdx_sync", "mdx_table_words",
    "mdx_finish_device", "mdx_finish", "mdx_reset", "mdx_timing_enable", "mdx_timing_read",
    "mdx_table_mode", "mdx_genome_composition", "mdx_rescale_set_model", "mdx_rescale_host",
    "mdx_rescale_summary_words", "mdx_rescale_summary",
    "mdx_comm_unique_id", "mdx_comm_init", "mdx_comm_adopt", "mdx_comm_size", "mdx_finish_allreduce",
    "mdx_rescale_device", "mdx_tabulate_rescale_device", "mdx_rescale_timing_read", "mdx_fused_launches",
    "mdx_bam_read", "mdx_bam_free", "mdx_bam_error", "mdx_bam_header_text", "mdx_bam_n_ref", "mdx_bam_ref_name",
    "mdx_bam_ref_length", "mdx_bam_batch", "mdx_bam_n_rg", "mdx_bam_rg_name", "mdx_bam_qnames",
    "mdx_bam_open", "mdx_bam_stream_header", "mdx_bam_next", "mdx_bam_close",
    "mdx_bam_stream_keep_raw", "mdx_bam_raw", "mdx_bam_patch_rescaled", "mdx_bam_qmin",
    "mdx_ctx_stream", "mdx_gbam_open", "mdx_gbam_header", "mdx_gbam_error", "mdx_gbam_configure", "mdx_gbam_next",
    "mdx_gbam_at_end", "mdx_gbam_close", "mdx_gbam_set_min_basequal", "mdx_gbam_missing_qualities",
    "mdx_gbam_inflate_blocks", "mdx_set_record_base", "mdx_pack_seq", "mdx_gbam_set_seq_format", "mdx_packed_launches", "mdx_geo_spec_launches",
    "mdx_gbam_skip", "mdx_comm_count", "mdx_gbam_tell", "mdx_gbam_fixups", "mdx_bam_seek", "mdx_libsorts",
    "mdx_gbam_view_flags", "mdx_gbam_view_set_flags",
    "mdx_rescale_patches_device", "mdx_tabulate_rescale_patches_device", "mdx_rescale_expand_device", "mdx_mr_round", "mdx_batch_fold", "mdx_bgzf_deflate",
    "mdx_gbam_rescale_slab", "mdx_gbam_write_rescaled", "mdx_gbam_record_name", "mdx_gbam_kept_bound", "mdx_gbam_write_kept",
    "mdx_gbam_kept_bound_tagged", "mdx_gbam_write_kept_tagged", "mdx_gbam_kept_index", "mdx_gbam_kept_index_linear", "mdx_gbam_set_kept_mask", "mdx_gbam_kept_mask_counts",
    "mdx_gbam_set_kept_md", "mdx_gbam_kept_md_counts", "mdx_gbam_kept_bound_md", "mdx_strata_pmd_keep_scores", "mdx_strata_pmd_scores",
    "mdx_fasta_index", "mdx_set_reference_fasta", "mdx_fasta_load_stats", "mdx_reference_fetch", "mdx_host_threads", "mdx_host_pool_threads", "mdx_warm",
    "mdx_source_open", "mdx_source_error", "mdx_source_is_stream", "mdx_source_peek", "mdx_source_read", "mdx_source_close",
    "mdx_bam_read_source", "mdx_bam_open_source", "mdx_gbam_open_source",
    "mdx_source_seek", "mdx_gsam_open", "mdx_gsam_open_source", "mdx_gsam_header", "mdx_gsam_error", "mdx_gsam_configure",
    "mdx_gsam_set_seq_format", "mdx_gsam_set_min_basequal", "mdx_gsam_next", "mdx_gsam_at_end", "mdx_gsam_tell",
    "mdx_gsam_view_flags", "mdx_gsam_view_set_flags", "mdx_gsam_missing_qualities", "mdx_gsam_close",
    "mdx_gsam_is_bgzf", "mdx_gsam_tell_bgzf",
    "mdx_last_launch_geometry",
    "mdx_set_strata", "mdx_set_strata_regions", "mdx_set_strata_damage", "mdx_set_strata_pmd", "mdx_strata_pmd_histogram", "mdx_strata_pmd_unqualified", "mdx_strata_groups", "mdx_strata_kept", "mdx_merged_words", "mdx_finish_merged", "mdx_finish_merged_host", "mdx_lgd_copies",
    "mdx_stats_loglik", "mdx_stats_run", "mdx_stats_pmat",
    "mdx_bam_apply_record_filter", "mdx_gbam_set_record_filter", "mdx_gbam_filter_counts", "mdx_gsam_set_record_filter",
    "mdx_gsam_filter_counts",
    "mdx_dedup_begin", "mdx_dedup_mark", "mdx_dedup_counts", "mdx_dedup_histogram", "mdx_dedup_info",
    "mdx_depth_begin", "mdx_depth_add", "mdx_depth_finish", "mdx_depth_runs", "mdx_depth_fetch", "mdx_depth_info", "mdx_depth_regions",
    "mdx_pileup_begin", "mdx_pileup_add", "mdx_pileup_finish", "mdx_pileup_info",
    "mdx_pileup_likelihoods_begin", "mdx_pileup_likelihoods_finish", "mdx_pileup_likelihoods_damage_begin",
)

SEQ_ASCII, SEQ_4BIT, SEQ_4BITQ = 0, 1, 2      # include/mdx.h MDX_SEQ_*


class MdxPileupConfig(ctypes.Structure):
    """include/mdx.h ``mdx_pileup_config``."""
    _fields_ = [("min_basequal", ctypes.c_int32), ("mask5", ctypes.c_int32), ("mask3", ctypes.c_int32), ("call", ctypes.c_int32),
                ("min_depth", ctypes.c_int32), ("single_strand", ctypes.c_int32), ("seed", ctypes.c_uint64)]


class MdxConfig(ctypes.Structure):
    _fields_ = [("length", ctypes.c_int32), ("around", ctypes.c_int32),
                ("minqual", ctypes.c_int32), ("nlib", ctypes.c_int32),
                ("lgd_max", ctypes.c_int32), ("device", ctypes.c_int32),
                ("lgd_over_cap", ctypes.c_int64)]


class MdxBatch(ctypes.Structure):
    _fields_ = [("n_reads", ctypes.c_int64), ("n_cigar", ctypes.c_int64),
                ("n_bases", ctypes.c_int64),
                ("flag", ctypes.c_void_p), ("lib", ctypes.c_void_p), ("tid", ctypes.c_void_p),
                ("pos", ctypes.c_void_p), ("tlen", ctypes.c_void_p),
                ("cigar_off", ctypes.c_void_p), ("cigar", ctypes.c_void_p),
                ("seq_off", ctypes.c_void_p), ("seq", ctypes.c_void_p),
                ("qual", ctypes.c_void_p),
                ("seq_format", ctypes.c_int32), ("reserved", ctypes.c_int32), ("lowq", ctypes.c_void_p),
                ("libsort", ctypes.c_void_p)]


class MdxError(RuntimeError):
    def __init__(self, code, message):
        super().__init__("libmdx error %d: %s" % (code, message))
        self.code = code


class BadReadError(ValueError):
    """A record the reference itself cannot process, e.g. an alignment running past the end
    of its contig, where pysam's ``FastaFile.fetch`` raises ``ValueError`` (align.py:33)."""

    def __init__(self, read_index, message):
        super().__init__("invalid coordinates or record at batch index %d: %s"
                         % (read_index, message))
        self.read_index = read_index


def load_library(path=None):
    """Load libmdx.so; raises (never falls back) when it has not been built."""
    global _lib
    if _lib is not None and path is None:
        return _lib
    # (MDX_LIBPATH: another build of the library — the A/B variants of tools/mkvariant.sh)
    p = pathlib.Path(path) if path else pathlib.Path(os.environ.get("MDX_LIBPATH") or _LIBPATH)
    if not p.exists():
        raise RuntimeError("%s is missing: build it with `python -m mapdamage_amd.build` "
                           "(hipcc, gfx950); there is no CPU fallback" % p)
    lib = ctypes.CDLL(str(p))
    lib.mdx_strerror.restype = ctypes.c_char_p
    lib.mdx_last_error.restype = ctypes.c_char_p
    lib.mdx_last_error.argtypes = [ctypes.c_void_p]
    lib.mdx_table_words.restype = ctypes.c_int64
    lib.mdx_table_words.argtypes = [ctypes.c_void_p]
    lib.mdx_destroy.restype = None
    lib.mdx_destroy.argtypes = [ctypes.c_void_p]
    for name in ("mdx_set_stream", "mdx_set_reference", "mdx_batch_upload", "mdx_batch_free",
                 "mdx_tabulate_host", "mdx_tabulate_device", "mdx_sync", "mdx_finish_device",
                 "mdx_finish", "mdx_reset", "mdx_timing_enable", "mdx_timing_read",
                 "mdx_table_mode", "mdx_genome_composition", "mdx_rescale_set_model", "mdx_rescale_host",
                 "mdx_rescale_summary", "mdx_comm_unique_id", "mdx_comm_init", "mdx_comm_adopt", "mdx_comm_size",
                 "mdx_finish_allreduce", "mdx_rescale_device", "mdx_tabulate_rescale_device", "mdx_rescale_timing_read",
                 "mdx_set_record_base"):
        getattr(lib, name).restype = ctypes.c_int
    lib.mdx_comm_size.argtypes = [ctypes.c_void_p]
    lib.mdx_comm_count.argtypes = [ctypes.c_void_p]
    lib.mdx_comm_adopt.argtypes = [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_int32, ctypes.c_int32]
    lib.mdx_rescale_summary_words.restype = ctypes.c_int64
    lib.mdx_rescale_summary_words.argtypes = [ctypes.c_void_p]
    lib.mdx_fused_launches.restype = ctypes.c_int64
    lib.mdx_fused_launches.argtypes = [ctypes.c_void_p]
    lib.mdx_packed_launches.restype = ctypes.c_int64
    lib.mdx_packed_launches.argtypes = [ctypes.c_void_p]
    lib.mdx_geo_spec_launches.restype = ctypes.c_int64
    lib.mdx_geo_spec_launches.argtypes = [ctypes.c_void_p]
    lib.mdx_libsorts.restype = ctypes.c_int64
    lib.mdx_libsorts.argtypes = [ctypes.c_void_p]
    lib.mdx_last_launch_geometry.restype = ctypes.c_int
    lib.mdx_last_launch_geometry.argtypes = [ctypes.c_void_p, ctypes.c_void_p]
    for name in ("mdx_bam_error", "mdx_bam_header_text", "mdx_bam_ref_name", "mdx_bam_rg_name"):
        getattr(lib, name).restype = ctypes.c_char_p
    lib.mdx_bam_qnames.restype = ctypes.c_void_p
    lib.mdx_bam_qmin.restype = ctypes.c_void_p
    lib.mdx_bam_qmin.argtypes = [ctypes.c_void_p]
    lib.mdx_bam_ref_length.restype = ctypes.c_int64
    lib.mdx_bam_free.restype = None
    for name in ("mdx_bam_error", "mdx_bam_header_text", "mdx_bam_n_ref", "mdx_bam_n_rg", "mdx_bam_free"):
        getattr(lib, name).argtypes = [ctypes.c_void_p]
    for name in ("mdx_bam_ref_name", "mdx_bam_ref_length", "mdx_bam_rg_name"):
        getattr(lib, name).argtypes = [ctypes.c_void_p, ctypes.c_int32]
    lib.mdx_bam_stream_header.restype = ctypes.c_void_p
    lib.mdx_bam_stream_header.argtypes = [ctypes.c_void_p]
    lib.mdx_bam_next.argtypes = [ctypes.c_void_p, ctypes.c_int64, ctypes.c_void_p]
    lib.mdx_bam_close.restype = None
    lib.mdx_bam_close.argtypes = [ctypes.c_void_p]
    lib.mdx_gbam_open.argtypes = [ctypes.c_void_p, ctypes.c_char_p, ctypes.c_void_p]
    lib.mdx_gbam_header.restype = ctypes.c_void_p
    lib.mdx_gbam_header.argtypes = [ctypes.c_void_p]
    lib.mdx_gbam_error.restype = ctypes.c_char_p
    lib.mdx_gbam_error.argtypes = [ctypes.c_void_p]
    lib.mdx_gbam_configure.argtypes = [ctypes.c_void_p, ctypes.c_int32, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_int32,
                                       ctypes.c_int, ctypes.c_int]
    lib.mdx_gbam_next.argtypes = [ctypes.c_void_p, ctypes.c_int64, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p]
    lib.mdx_gbam_at_end.argtypes = [ctypes.c_void_p]
    lib.mdx_gbam_skip.argtypes = [ctypes.c_void_p, ctypes.c_int64]
    lib.mdx_gbam_tell.argtypes = [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p]
    lib.mdx_gbam_fixups.argtypes = [ctypes.c_void_p]
    lib.mdx_bam_seek.argtypes = [ctypes.c_void_p, ctypes.c_int64, ctypes.c_int64]
    lib.mdx_gbam_set_min_basequal.argtypes = [ctypes.c_void_p, ctypes.c_int32]
    lib.mdx_gbam_set_seq_format.argtypes = [ctypes.c_void_p, ctypes.c_int32]
    lib.mdx_pack_seq.restype = ctypes.c_int
    lib.mdx_pack_seq.argtypes = [ctypes.c_void_p, ctypes.c_int64, ctypes.c_void_p, ctypes.c_int32]
    lib.mdx_gbam_missing_qualities.argtypes = [ctypes.c_void_p]
    for name in ("mdx_gbam_set_record_filter", "mdx_gbam_filter_counts", "mdx_gsam_set_record_filter", "mdx_gsam_filter_counts"):
        getattr(lib, name).argtypes = [ctypes.c_void_p, ctypes.c_void_p]
    lib.mdx_bam_apply_record_filter.argtypes = [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p]
    lib.mdx_gbam_close.restype = None
    lib.mdx_gbam_close.argtypes = [ctypes.c_void_p]
    lib.mdx_fasta_index.argtypes = [ctypes.c_char_p, ctypes.c_char_p, ctypes.c_int32]
    lib.mdx_fasta_load_stats.argtypes = [ctypes.c_void_p]
    lib.mdx_set_reference_fasta.argtypes = [ctypes.c_void_p, ctypes.c_char_p, ctypes.c_int32, ctypes.c_void_p, ctypes.c_int32,
                                            ctypes.c_void_p]
    lib.mdx_reference_fetch.argtypes = [ctypes.c_void_p, ctypes.c_int32, ctypes.c_int64, ctypes.c_int64, ctypes.c_void_p]
    lib.mdx_warm.argtypes = [ctypes.c_int32, ctypes.c_int64]
    lib.mdx_source_open.argtypes = [ctypes.c_char_p, ctypes.c_void_p]
    lib.mdx_source_error.restype = ctypes.c_char_p
    lib.mdx_source_error.argtypes = [ctypes.c_void_p]
    lib.mdx_source_is_stream.argtypes = [ctypes.c_void_p]
    lib.mdx_source_peek.argtypes = [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_int32, ctypes.c_void_p]
    lib.mdx_source_read.restype = ctypes.c_int64
    lib.mdx_source_read.argtypes = [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_int64]
    lib.mdx_source_close.restype = None
    lib.mdx_source_close.argtypes = [ctypes.c_void_p]
    lib.mdx_bam_read_source.argtypes = [ctypes.c_void_p, ctypes.c_int, ctypes.c_void_p]
    lib.mdx_bam_open_source.argtypes = [ctypes.c_void_p, ctypes.c_int, ctypes.c_void_p]
    lib.mdx_gbam_open_source.argtypes = [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p]
    lib.mdx_set_strata.argtypes = [ctypes.c_void_p, ctypes.c_int32, ctypes.c_void_p, ctypes.c_int32]
    lib.mdx_set_strata_regions.argtypes = [ctypes.c_void_p, ctypes.c_int32, ctypes.c_int32, ctypes.c_void_p, ctypes.c_void_p,
                                           ctypes.c_void_p, ctypes.c_void_p, ctypes.c_int32]
    lib.mdx_set_strata_damage.argtypes = [ctypes.c_void_p, ctypes.c_int32, ctypes.c_int32]
    lib.mdx_set_strata_pmd.argtypes = [ctypes.c_void_p, ctypes.c_int32, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_int32]
    lib.mdx_strata_pmd_histogram.argtypes = [ctypes.c_void_p, ctypes.c_void_p]
    lib.mdx_strata_pmd_unqualified.argtypes = [ctypes.c_void_p, ctypes.c_void_p]
    lib.mdx_strata_pmd_keep_scores.argtypes = [ctypes.c_void_p, ctypes.c_int32]
    lib.mdx_strata_pmd_scores.argtypes = [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_int64]
    lib.mdx_strata_groups.argtypes = [ctypes.c_void_p]
    lib.mdx_strata_kept.argtypes = [ctypes.c_void_p, ctypes.c_void_p]
    lib.mdx_merged_words.restype = ctypes.c_int64
    lib.mdx_merged_words.argtypes = [ctypes.c_void_p]
    lib.mdx_finish_merged.argtypes = [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p]
    lib.mdx_finish_merged_host.argtypes = [ctypes.c_void_p, ctypes.c_void_p]
    lib.mdx_lgd_copies.argtypes = [ctypes.c_void_p]
    lib.mdx_dedup_begin.argtypes = [ctypes.c_void_p, ctypes.c_int32, ctypes.c_int64]
    for name in ("mdx_dedup_mark", "mdx_dedup_counts", "mdx_dedup_histogram", "mdx_dedup_info"):
        getattr(lib, name).argtypes = [ctypes.c_void_p, ctypes.c_void_p]
    lib.mdx_depth_begin.argtypes = [ctypes.c_void_p]
    lib.mdx_depth_add.argtypes = [ctypes.c_void_p, ctypes.c_void_p]
    lib.mdx_depth_finish.argtypes = [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p]
    lib.mdx_depth_runs.argtypes = [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_int64,
                                   ctypes.c_void_p]
    lib.mdx_depth_fetch.argtypes = [ctypes.c_void_p, ctypes.c_int32, ctypes.c_int64, ctypes.c_int64, ctypes.c_void_p]
    lib.mdx_depth_info.argtypes = [ctypes.c_void_p, ctypes.c_void_p]
    lib.mdx_depth_regions.argtypes = [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p]
    lib.mdx_pileup_begin.argtypes = [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_int32, ctypes.c_void_p]
    lib.mdx_pileup_add.argtypes = [ctypes.c_void_p, ctypes.c_void_p]
    lib.mdx_pileup_finish.argtypes = [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p]
    lib.mdx_pileup_info.argtypes = [ctypes.c_void_p, ctypes.c_void_p]
    lib.mdx_pileup_likelihoods_begin.argtypes = [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_int32]
    lib.mdx_pileup_likelihoods_damage_begin.argtypes = [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_int32, ctypes.c_int32]
    lib.mdx_pileup_likelihoods_finish.argtypes = [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p]
    if path is None:
        _lib = lib
    return lib


def _ptr(a):
    return None if a is None else ctypes.c_void_p(a.ctypes.data)


def pack_seq(seq, threads=None):
    """ASCII SEQ bytes -> the 4-bit column of ``MDX_SEQ_4BIT`` (include/mdx.h): two bases per byte, low nibble first,
    1 = A, 2 = C, 4 = T, 8 = G, 0 = anything else — all the reference's loop distinguishes (statistics.py:27, 101)."""
    seq = np.ascontiguousarray(seq, dtype=np.uint8)
    out = np.empty((seq.shape[0] + 1) // 2, np.uint8)
    if threads is None:
        # (the control group's quota, not the hardware's thread count: mdx_pack_seq with 0 would start one thread per hardware thread)
        from .sam import usable_cpus
        threads = min(64, usable_cpus())
    rc = load_library().mdx_pack_seq(_ptr(seq), ctypes.c_int64(seq.shape[0]), _ptr(out), ctypes.c_int32(threads))
    if rc != 0:
        raise MdxError(rc, "mdx_pack_seq")
    return out


def _host_batch(batch: ReadBatch, packed=False):
    b = MdxBatch()
    b.n_reads = batch.n
    b.n_cigar = int(batch.cigar.shape[0])
    b.n_bases = int(batch.seq.shape[0])
    keep = []
    for name in ("flag", "lib", "tid", "pos", "tlen", "cigar_off", "cigar", "seq_off", "seq"):
        arr = np.ascontiguousarray(getattr(batch, name))
        if name == "seq" and packed:
            arr = pack_seq(arr)
            b.seq_format = SEQ_4BIT
        setattr(b, name, arr.ctypes.data)
        keep.append(arr)
    if batch.qual is not None:
        q = np.ascontiguousarray(batch.qual)
        b.qual = q.ctypes.data
        keep.append(q)
    b._keep = keep  # the columns must outlive the call
    return b


class DeviceBatch:
    """A batch resident in HBM (allocated by the library)."""

    def __init__(self, engine, dev, n_reads, n_bases, n_cigar):
        self._engine = engine
        self.dev = dev
        self.n = n_reads
        self.n_bases = n_bases
        self.n_cigar = n_cigar

    def free(self):
        if self.dev is not None and self._engine._ctx:
            self._engine._lib.mdx_batch_free(self._engine._ctx, ctypes.byref(self.dev))
        self.dev = None


class DamageEngine:
    """Device-side counterpart of MisincorporationRates + DNAComposition + FragmentLengths.

    ``libraries``: list of (sample, library) tuples indexed by the ``lib`` column (unique
    libraries in header order, or ``[("*", "*")]`` for --merge-libraries).

    ``groups``: names of groups of reference sequences — the engine then keeps one table set per (library, group), a
    *stratum* (include/mdx.h ``mdx_set_strata``): ``set_strata(group_of_tid)`` says which group each sequence of the
    header belongs to (or ``set_strata_regions(...)`` which group each region of a BED file does, or ``set_strata_damage(...)``
    that the groups are ``DAMAGE_GROUPS``, told by the substitutions at the record's own ends, or ``set_strata_pmd(...)`` that
    they are the intervals between thresholds of the record's post-mortem damage score), the batches keep naming
    the library in their ``lib`` column, and ``finish()`` returns a ``tables.StratifiedTables``.  ``libraries`` then holds one entry per stratum, library-major (``base_libraries`` the
    caller's list)."""

    MAX_TABLES = 65535      # the 16-bit library column, 0xFFFF being the record without a library

    # the form in which ``upload`` / ``tabulate`` hand a host batch's SEQ column over when the caller does not say
    # (False: ASCII as it stands, True: packed to 4 bits first); the tests run every parity case through both
    # (MDX_SEQ_4BIT=1 in the environment: packed, for the profiling scripts under tools/)
    default_packed = os.environ.get("MDX_SEQ_4BIT", "") == "1"

    def __init__(self, libraries, length=70, around=10, minqual=0, lgd_max=65536, device=0,
                 lgd_over_cap=1 << 20, groups=None):
        self.base_libraries = [tuple(x) for x in libraries]
        self.groups = None if groups is None else [str(g) for g in groups]
        if self.groups is not None and not self.groups:
            raise ValueError("groups: at least one group of reference sequences")
        n_tables = len(self.base_libraries) * (len(self.groups) if self.groups is not None else 1)
        if n_tables > self.MAX_TABLES:
            raise ValueError("%d libraries x %d reference groups = %d tables; the 16-bit library column names at most %d"
                             % (len(self.base_libraries), len(self.groups or [None]), n_tables, self.MAX_TABLES))
        self._lib = load_library()
        self.strata_kind = None        # "reference", "regions", "damage" or "pmd" once a set_strata* call succeeded (groupings.KINDS)
        self.libraries = [lib for lib in self.base_libraries for _ in (self.groups or [None])]
        self.length, self.around, self.minqual, self.lgd_max = length, around, minqual, lgd_max
        self.lgd_over_cap = lgd_over_cap
        cfg = MdxConfig(length, around, minqual, len(self.libraries), lgd_max, device, lgd_over_cap)
        ctx = ctypes.c_void_p()
        rc = self._lib.mdx_create(ctypes.byref(cfg), ctypes.byref(ctx))
        self._ctx = ctx if ctx.value else None
        if rc != 0:
            msg = self._lib.mdx_strerror(rc).decode()
            if self._ctx:
                msg += ": " + self._lib.mdx_last_error(self._ctx).decode()
                self._lib.mdx_destroy(self._ctx)
                self._ctx = None
            raise MdxError(rc, msg + " (a HIP device is required; there is no CPU fallback)")

    # ------------------------------------------------------------------ plumbing
    def _check(self, rc):
        if rc != 0:
            raise MdxError(rc, self._lib.mdx_last_error(self._ctx).decode()
                           or self._lib.mdx_strerror(rc).decode())

    def close(self):
        if self._ctx:
            # (a device decode stream hands its arena back to the context when it closes — mdx_gbam_close — so the streams
            # opened on this engine are closed before the context goes)
            for stream in list(getattr(self, "_streams", ())):
                stream.close()
            self._lib.mdx_destroy(self._ctx)
            self._ctx = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()

    @property
    def table_mode(self):
        return "lds" if self._lib.mdx_table_mode(self._ctx) == 0 else "global"

    def set_stream(self, hip_stream):
        self._check(self._lib.mdx_set_stream(self._ctx, ctypes.c_void_p(hip_stream or 0)))

    # ------------------------------------------------------------------ inputs
    def set_strata(self, group_of_tid):
        """``group_of_tid[t]``: index into ``groups`` of sequence ``t`` of the header (include/mdx.h ``mdx_set_strata``);
        before the first ``tabulate`` / ``upload``."""
        if self.groups is None:
            raise ValueError("set_strata: the engine was made without groups")
        m = np.ascontiguousarray(group_of_tid, dtype=np.int32)
        self._check(self._lib.mdx_set_strata(self._ctx, ctypes.c_int32(len(self.groups)), _ptr(m), ctypes.c_int32(m.shape[0])))
        self.strata_kind = "reference"

    def set_strata_regions(self, iv_off, iv_start, iv_end, iv_group, rest_group=None):
        """The group of a record from a set of regions (include/mdx.h ``mdx_set_strata_regions``): the intervals of sequence
        ``t`` are ``iv_off[t]:iv_off[t + 1]`` of ``iv_start, iv_end, iv_group`` (0-based, half-open, sorted and disjoint
        within a sequence, ``iv_group`` an index into ``groups``); a record that overlaps none goes to ``rest_group`` (default:
        the last group).  Before the first ``tabulate`` / ``upload``."""
        if self.groups is None:
            raise ValueError("set_strata_regions: the engine was made without groups")
        off = np.ascontiguousarray(iv_off, dtype=np.int64)
        cols = [np.ascontiguousarray(a, dtype=np.int32) for a in (iv_start, iv_end, iv_group)]
        if off.ndim != 1 or off.shape[0] < 2 or any(a.ndim != 1 or a.shape[0] != cols[0].shape[0] for a in cols) \
                or int(off[-1]) != cols[0].shape[0]:
            raise ValueError("set_strata_regions: iv_off must hold one entry per sequence and one more, its last the "
                             "length of the three interval columns")
        rest = len(self.groups) - 1 if rest_group is None else int(rest_group)
        self._check(self._lib.mdx_set_strata_regions(self._ctx, ctypes.c_int32(len(self.groups)), ctypes.c_int32(off.shape[0] - 1),
                                                     _ptr(off), _ptr(cols[0]), _ptr(cols[1]), _ptr(cols[2]), ctypes.c_int32(rest)))
        self.strata_kind = "regions"
        self._n_intervals = int(cols[0].shape[0])

    DAMAGE_GROUPS = ["none", "5p", "3p", "both"]

    def set_strata_damage(self, positions=1, single_stranded=False):
        """The group of a record from the damage its own ends show (include/mdx.h ``mdx_set_strata_damage``): 5p-damaged if
        the reference's 5p update would add to C>T within the first ``positions`` positions, 3p-damaged if its 3p update
        would add to G>A there (``single_stranded``: C>T).  The engine's ``groups`` must be ``DAMAGE_GROUPS``.  Before the
        first ``tabulate``; the key reads the reference, so ``set_reference`` comes before ``upload``."""
        if self.groups != self.DAMAGE_GROUPS:
            raise ValueError("set_strata_damage: the engine must be made with groups=%r" % (self.DAMAGE_GROUPS,))
        self._check(self._lib.mdx_set_strata_damage(self._ctx, ctypes.c_int32(int(positions)), ctypes.c_int32(1 if single_stranded else 0)))
        self.strata_kind = "damage"

    def set_strata_pmd(self, thresholds, model=(0.3, 0.01, 0.001), single_stranded=False, keep_scores=False):
        """The group of a record from its post-mortem damage score (include/mdx.h ``mdx_set_strata_pmd``; the rule is
        ``csrc/mdx_pmd_key.h``): the number of ``thresholds`` (1 to 15, strictly increasing) the score reaches, under the
        model ``(p, C, pi)`` of ``pmd.term_table``.  The engine's ``groups`` number ``len(thresholds) + 1``
        (``pmd.group_names``), and it has no ``minqual``.  Before the first ``tabulate``; the key reads the reference, so
        ``set_reference`` comes before ``upload``; the batches bring their qualities if these are to count.
        ``keep_scores``: the key kernel also leaves every record's score as a float32 (``keep_pmd_scores``)."""
        from . import pmd
        ts = pmd.check_thresholds(thresholds)
        if self.groups is None or len(self.groups) != len(ts) + 1:
            raise ValueError("set_strata_pmd: %d thresholds make %d groups; the engine was made with %s"
                             % (len(ts), len(ts) + 1, "none" if self.groups is None else "%d" % len(self.groups)))
        fx = np.array([pmd.threshold_fx(t) for t in ts], np.int64)
        terms = np.ascontiguousarray(pmd.term_table(*model), np.int32)
        self._check(self._lib.mdx_set_strata_pmd(self._ctx, ctypes.c_int32(len(ts)), _ptr(fx), _ptr(terms),
                                                 ctypes.c_int32(1 if single_stranded else 0)))
        self.strata_kind = "pmd"
        if keep_scores:
            self.keep_pmd_scores(True)

    def keep_pmd_scores(self, on=True):
        """From the next keyed batch on, keep the scores of the batch keyed last on the device (include/mdx.h
        ``mdx_strata_pmd_keep_scores``): what ``pmd_scores()`` fetches and the score tag of
        ``sam.GpuBamStream.write_kept`` is written from."""
        self._check(self._lib.mdx_strata_pmd_keep_scores(self._ctx, ctypes.c_int32(1 if on else 0)))

    def pmd_scores(self, n=None):
        """float32 [n]: the PMD scores of the ``n`` records of the batch tabulated last (default: as many as that batch had) (``mdx_strata_pmd_scores``) — the
        fixed-point score as the nearest float32, times 2^-24.  MdxError -3 without PMD strata, without ``keep_pmd_scores``,
        or behind a resident batch that brought its buckets."""
        n = getattr(self, "_last_n_reads", 0) if n is None else int(n)
        out = np.zeros(n, np.float32)
        self._check(self._lib.mdx_strata_pmd_scores(self._ctx, _ptr(out), ctypes.c_int64(int(n))))
        return out

    @property
    def pmd_strata(self):
        """The engine's strata are those of ``set_strata_pmd``: ``finish()`` brings the score histogram."""
        return self.strata_kind == "pmd"

    def pmd_histogram(self):
        """uint64 [base libraries][82]: the kept records of each library by their score (``mdx_strata_pmd_histogram``; bin
        ``b`` holds the scores of ``pmd.bin_edges(b)``)."""
        # (sized by the context's own count of libraries: its tables over its groups)
        hist = np.zeros((len(self.libraries) // max(1, int(self._lib.mdx_strata_groups(self._ctx))), 82), np.uint64)
        self._check(self._lib.mdx_strata_pmd_histogram(self._ctx, _ptr(hist)))
        return hist

    def pmd_unqualified(self):
        """How many of the histogram's records were scored without qualities (``mdx_strata_pmd_unqualified``)."""
        n = np.zeros(1, np.uint64)
        self._check(self._lib.mdx_strata_pmd_unqualified(self._ctx, _ptr(n)))
        return int(n[0])

    def strata_kept(self):
        """Records the flag filter kept, per stratum (library-major), of this engine's batches (``mdx_strata_kept``)."""
        kept = np.zeros(len(self.libraries), np.uint64)
        self._check(self._lib.mdx_strata_kept(self._ctx, _ptr(kept)))
        return kept

    def lgd_copies(self):
        """Copies of the dense fragment-length histogram this context keeps (``mdx_lgd_copies``; tests)."""
        return int(self._lib.mdx_lgd_copies(self._ctx))

    # ------------------------------------------------------------------ duplicate removal
    DUPLICATE_ENDS = ("both", "5p")
    DUPLICATE_BINS = 1024

    def _base_library_count(self):
        return len(self.libraries) // max(1, int(self._lib.mdx_strata_groups(self._ctx)))

    def dedup_begin(self, ends="both", expected_records=0):
        """From here on ``dedup_mark`` knows the records it has seen (include/mdx.h ``mdx_dedup_begin``): ``ends`` "both" — a
        molecule is (library, sequence, strand, both unclipped ends) — or "5p" — ... the 5' end alone."""
        if ends not in self.DUPLICATE_ENDS:
            raise ValueError("dedup_begin: ends is one of %s" % ", ".join(self.DUPLICATE_ENDS))
        self._check(self._lib.mdx_dedup_begin(self._ctx, ctypes.c_int32(self.DUPLICATE_ENDS.index(ends)), ctypes.c_int64(int(expected_records))))

    def dedup_mark(self, view):
        """0x400 into the flag column of a device batch (an ``MdxBatch`` of device pointers, or a ``DeviceBatch``) where the
        record is a later copy of a molecule seen before, in this batch or an earlier one (``mdx_dedup_mark``): enqueued."""
        dev = view.dev if isinstance(view, DeviceBatch) else view
        self._check(self._lib.mdx_dedup_mark(self._ctx, ctypes.byref(dev)))

    def dedup_counts(self):
        """uint64 [base libraries][4]: examined, duplicates, not examined because paired, not examined otherwise (``mdx_dedup_counts``)."""
        out = np.zeros((self._base_library_count(), 4), np.uint64)
        self._check(self._lib.mdx_dedup_counts(self._ctx, _ptr(out)))
        return out

    def dedup_histogram(self):
        """uint64 [base libraries][1024]: molecules seen ``c`` times in column ``c - 1``, the last column ``c >= 1024`` (``mdx_dedup_histogram``)."""
        out = np.zeros((self._base_library_count(), self.DUPLICATE_BINS), np.uint64)
        self._check(self._lib.mdx_dedup_histogram(self._ctx, _ptr(out)))
        return out

    def dedup_info(self):
        """The set's table (``mdx_dedup_info``): slots, growths, longest and summed walk of an insert, examined records, bytes of HBM,
        the records a block of the stage's kernels takes and those a round of its one-block prefix sum takes."""
        out = np.zeros(8, np.uint64)
        self._check(self._lib.mdx_dedup_info(self._ctx, _ptr(out)))
        return dict(zip(("slots", "growths", "longest_probe", "probes", "examined", "bytes", "block_records", "scan_records"),
                        (int(x) for x in out)))

    # ------------------------------------------------------------------ depth of coverage
    DEPTH_BINS = 1024

    def depth_begin(self):
        """The zeroed accumulator over the resident reference, 4 bytes per base (include/mdx.h ``mdx_depth_begin``); a second
        call zeroes it."""
        self._check(self._lib.mdx_depth_begin(self._ctx))

    def depth_add(self, view):
        """The covered intervals of a device batch's counted records into the accumulator (``mdx_depth_add``): enqueued.  The
        flag column is read as it stands, so behind ``dedup_mark`` the later copies add nothing."""
        dev = view.dev if isinstance(view, DeviceBatch) else view
        self._check(self._lib.mdx_depth_add(self._ctx, ctypes.byref(dev)))

    def depth_finish(self):
        """``(per_contig, hist, counts)`` (``mdx_depth_finish``): uint64 [sequences][4] — counted records, covered bases,
        aligned bases, largest depth —, uint64 [1024] — bases at depth ``d``, the last bin ``>= 1023`` — and a dict of the
        records counted, those outside their sequence, the intervals and the runs of depth > 0."""
        per_contig = np.zeros((getattr(self, "_n_contig", 0), 4), np.uint64)
        hist = np.zeros(self.DEPTH_BINS, np.uint64)
        counts = np.zeros(4, np.uint64)
        self._check(self._lib.mdx_depth_finish(self._ctx, _ptr(per_contig), _ptr(hist), _ptr(counts)))
        return per_contig, hist, dict(zip(("counted", "outside", "intervals", "runs"), (int(x) for x in counts)))

    def depth_runs(self):
        """``(tid, start, end, depth)``: the maximal runs of equal depth > 0 in reference order (``mdx_depth_runs``)."""
        n = ctypes.c_int64(0)
        rc = self._lib.mdx_depth_runs(self._ctx, None, None, None, None, ctypes.c_int64(0), ctypes.byref(n))
        if rc != 0 and n.value == 0:
            self._check(rc)
        cap = max(1, n.value)
        tid, start, end, depth = np.zeros(cap, np.int32), np.zeros(cap, np.int64), np.zeros(cap, np.int64), np.zeros(cap, np.uint32)
        self._check(self._lib.mdx_depth_runs(self._ctx, _ptr(tid), _ptr(start), _ptr(end), _ptr(depth), ctypes.c_int64(cap), ctypes.byref(n)))
        return tid[:n.value], start[:n.value], end[:n.value], depth[:n.value]

    def depth_fetch(self, tid, start, end):
        """uint32 depths of bases ``[start, end)`` of sequence ``tid`` as the accumulator holds them (``mdx_depth_fetch``; tests)."""
        out = np.zeros(max(0, end - start), np.uint32)
        self._check(self._lib.mdx_depth_fetch(self._ctx, ctypes.c_int32(tid), ctypes.c_int64(start), ctypes.c_int64(end), _ptr(out) if len(out) else _ptr(np.zeros(1, np.uint32))))
        return out

    def depth_info(self):
        """The stage's sizes (``mdx_depth_info``): the records a block of the add kernel takes, the elements of a tile, the
        tiles a round of the one-block scan takes, the bytes of HBM held."""
        out = np.zeros(4, np.uint64)
        self._check(self._lib.mdx_depth_info(self._ctx, _ptr(out)))
        return dict(zip(("block_records", "tile", "round_tiles", "bytes"), (int(x) for x in out)))

    def depth_regions(self):
        """``(per_interval, per_group, group_hist)`` (``mdx_depth_regions``): the depth parted by the intervals of
        ``set_strata_regions``, base by base.  uint64 [intervals][4] — covered bases, aligned bases, smallest and largest
        depth —, uint64 [groups][4] — bases, covered, aligned, largest depth, the rest group's row also what no interval
        holds — and uint64 [groups][1024], a group's bases at depth ``d`` binned as ``depth_finish`` bins."""
        n_iv, n_groups = getattr(self, "_n_intervals", 0), len(self.groups or ())
        per_interval = np.zeros((n_iv, 4), np.uint64)
        per_group = np.zeros((n_groups, 4), np.uint64)
        group_hist = np.zeros((n_groups, self.DEPTH_BINS), np.uint64)
        self._check(self._lib.mdx_depth_regions(self._ctx, _ptr(per_interval) if n_iv else None, _ptr(per_group) if n_groups else None,
                                                _ptr(group_hist) if n_groups else None))
        return per_interval, per_group, group_hist

    # ------------------------------------------------------------------ allele counts at listed sites
    PILEUP_COUNTERS = 12
    PILEUP_CALLS = {"none": 0, "random": 1, "majority": 2}      # include/mdx.h MDX_PILEUP_CALL_*

    def pileup_begin(self, site_pos, site_off, alleles=None, min_basequal=0, mask_ends=(0, 0), call="random", seed=0, min_depth=1,
                     single_strand=False):
        """The sites resident and their zeroed counters, 48 bytes per site (include/mdx.h ``mdx_pileup_begin``).  ``site_pos``:
        0-based positions, strictly increasing inside each sequence's slice ``site_off[t]:site_off[t + 1]``; ``alleles``: uint8
        [sites][2], ref and alt as 0 .. 3 for A C G T, or None.  A second call starts from zero with the new sites."""
        site_pos = np.ascontiguousarray(site_pos, np.int32)
        site_off = np.ascontiguousarray(site_off, np.int64)
        if alleles is not None:
            alleles = np.ascontiguousarray(alleles, np.uint8).reshape(-1, 2)
            if len(alleles) != len(site_pos):
                raise ValueError("pileup_begin: %d rows of alleles for %d sites" % (len(alleles), len(site_pos)))
        if len(site_off) < 2 or int(site_off[-1]) != len(site_pos):
            raise ValueError("pileup_begin: site_off does not end at the number of sites")
        cfg = MdxPileupConfig(int(min_basequal), int(mask_ends[0]), int(mask_ends[1]), self.PILEUP_CALLS[call], int(min_depth),
                              int(bool(single_strand)), int(seed) & 0xFFFFFFFFFFFFFFFF)
        self._check(self._lib.mdx_pileup_begin(self._ctx, ctypes.byref(cfg), _ptr(site_pos) if len(site_pos) else _ptr(np.zeros(1, np.int32)), _ptr(site_off),
                                               ctypes.c_int32(len(site_off) - 1), _ptr(alleles) if alleles is not None and len(alleles) else None))
        self._n_pileup_sites = len(site_pos)

    def pileup_add(self, view):
        """The (record, site) pairs of a device batch's counted records into the sites' counters (``mdx_pileup_add``): enqueued.
        The flag column is read as it stands, so behind ``dedup_mark`` the later copies add nothing."""
        dev = view.dev if isinstance(view, DeviceBatch) else view
        self._check(self._lib.mdx_pileup_add(self._ctx, ctypes.byref(dev)))

    def pileup_finish(self):
        """``(counters, refbase, call, depth, counts)`` (``mdx_pileup_finish``): uint32 [sites][12] — A+ C+ G+ T+ A- C- G- T-
        Deletions LowQual Other Masked —, the reference's letter and the call per site as bytes (``S1``; the call ``.`` under
        ``call="none"``), uint32 depths — the sum of the eight base counters — and a dict of the records counted, those outside
        their sequence, those over at least one site and the (record, site) pairs."""
        n = getattr(self, "_n_pileup_sites", 0)
        counters = np.zeros((max(1, n), self.PILEUP_COUNTERS), np.uint32)
        refbase, call, depth = np.zeros(max(1, n), "S1"), np.zeros(max(1, n), "S1"), np.zeros(max(1, n), np.uint32)
        counts = np.zeros(4, np.uint64)
        self._check(self._lib.mdx_pileup_finish(self._ctx, _ptr(counters), _ptr(refbase), _ptr(call), _ptr(depth), _ptr(counts)))
        return counters[:n], refbase[:n], call[:n], depth[:n], dict(zip(("counted", "outside", "over_a_site", "pairs"), (int(x) for x in counts)))

    def pileup_info(self):
        """The stage's sizes (``mdx_pileup_info``): the pairs the add kernel's list holds in a round, the records a block of it
        takes, the bytes of HBM held, the sites."""
        out = np.zeros(4, np.uint64)
        self._check(self._lib.mdx_pileup_info(self._ctx, _ptr(out)))
        return dict(zip(("list_pairs", "block_records", "bytes", "sites"), (int(x) for x in out)))

    PILEUP_GENOTYPES = 10       # AA AC AG AT CC CG CT GG GT TT
    PILEUP_SUMS = 24            # [2 strands][4 bases][HOM HET NO]

    def pileup_likelihoods_begin(self, table=None, noqual_quality=30):
        """The sites' zeroed sums beside their counters, 192 bytes per site (include/mdx.h ``mdx_pileup_likelihoods_begin``):
        behind ``pileup_begin``, in front of the first ``pileup_add``.  ``table``: int64 [94][3], the model's terms per quality
        (None: ``pileup.likelihood_table()``); ``noqual_quality``: the quality of a record without qualities, 1..93."""
        if table is None:
            from .pileup import likelihood_table
            table = likelihood_table()
        table = np.ascontiguousarray(table, np.int64)
        if table.shape != (94, 3):
            raise ValueError("pileup_likelihoods_begin: the table is %r, not (94, 3)" % (table.shape,))
        self._check(self._lib.mdx_pileup_likelihoods_begin(self._ctx, _ptr(table), ctypes.c_int32(int(noqual_quality))))
        self._pileup_sums = self.PILEUP_SUMS

    PILEUP_DAMAGE_SUMS = 20     # [2 strands][10 genotypes]

    def pileup_likelihoods_damage_begin(self, table, noqual_quality=30):
        """The sites' zeroed sums of the damage-aware model, 160 bytes per site (include/mdx.h
        ``mdx_pileup_likelihoods_damage_begin``): behind ``pileup_begin``, in front of the first ``pileup_add``, instead of
        ``pileup_likelihoods_begin``.  ``table``: int64 [2][K + 1][94][9], ``pileup.damage_likelihood_table(profile)``;
        ``noqual_quality``: the quality of a record without qualities, 1..93."""
        table = np.ascontiguousarray(table, np.int64)
        if table.ndim != 4 or table.shape[0] != 2 or table.shape[2:] != (94, 9):
            raise ValueError("pileup_likelihoods_damage_begin: the table is %r, not (2, K + 1, 94, 9)" % (table.shape,))
        self._check(self._lib.mdx_pileup_likelihoods_damage_begin(self._ctx, _ptr(table), ctypes.c_int32(table.shape[1]), ctypes.c_int32(int(noqual_quality))))
        self._pileup_sums = self.PILEUP_DAMAGE_SUMS

    def pileup_likelihoods_finish(self, with_sums=True):
        """``(sums, gl, best, bases, counts)`` (``mdx_pileup_likelihoods_finish``): int64 [sites][24] — the terms HOM HET NO
        summed per strand and base; behind ``pileup_likelihoods_damage_begin`` [sites][20], the ten genotypes' terms summed per
        strand; None without ``with_sums`` —, int64 [sites][10] — the ten genotypes' log likelihoods minus
        the site's largest, in units of 2^-24 —, the index of the best as uint8, the bases behind them as uint32, and a dict of
        the pairs that added and those of them from records without qualities."""
        n = getattr(self, "_n_pileup_sites", 0)
        sums = np.zeros((max(1, n), getattr(self, "_pileup_sums", self.PILEUP_SUMS)), np.int64) if with_sums else None
        gl = np.zeros((max(1, n), self.PILEUP_GENOTYPES), np.int64)
        best, bases, counts = np.zeros(max(1, n), np.uint8), np.zeros(max(1, n), np.uint32), np.zeros(2, np.uint64)
        self._check(self._lib.mdx_pileup_likelihoods_finish(self._ctx, _ptr(sums) if with_sums else None, _ptr(gl), _ptr(best), _ptr(bases), _ptr(counts)))
        return sums[:n] if with_sums else None, gl[:n], best[:n], bases[:n], dict(zip(("added", "without_qualities"), (int(x) for x in counts)))

    def set_reference(self, ref):
        """``ref``: a ``Reference`` (contigs in host memory) or a ``fasta.FastaOnDisk`` — the FASTA file itself, which the
        library sends to HBM as it lies on disk and strips of its line ends there (``mdx_set_reference_fasta``)."""
        path = getattr(ref, "path", None)
        self._n_contig = len(ref.names)
        if path is not None:
            names = [n.encode() for n in ref.names]
            arr = (ctypes.c_char_p * max(1, len(names)))(*names)
            lengths = np.zeros(max(1, len(names)), np.int64)
            self._check(self._lib.mdx_set_reference_fasta(self._ctx, str(path).encode(), ctypes.c_int32(len(names)), arr,
                                                          ctypes.c_int32(1 if ref.missing_ok else 0), _ptr(lengths)))
            ref.lengths = [int(x) for x in lengths[:len(names)]]
            return
        bases, offs = ref.concat()
        self._check(self._lib.mdx_set_reference(self._ctx, _ptr(bases), _ptr(offs),
                                                ctypes.c_int32(len(ref.names))))

    def fasta_load_stats(self):
        """What this thread's last ``set_reference`` of a ``FastaOnDisk`` read (``mdx_fasta_load_stats``): BGZF blocks of the
        file, blocks inflated on the device, slabs (or pieces of an uncompressed file) uploaded, bytes of the file uploaded."""
        out = np.zeros(4, np.int64)
        self._check(self._lib.mdx_fasta_load_stats(_ptr(out)))
        return dict(zip(("blocks", "inflated", "slabs", "bytes"), (int(x) for x in out)))

    def reference_fetch(self, tid, start, end):
        """``ref.fetch(chrom, start, end).upper()`` (main.py:180) as the kernels see it: the four bases, '-', and 'N' for
        every other symbol (tests)."""
        out = np.zeros(max(0, end - start), np.uint8)
        self._check(self._lib.mdx_reference_fetch(self._ctx, ctypes.c_int32(tid), ctypes.c_int64(start), ctypes.c_int64(end),
                                                  _ptr(out)))
        return out.tobytes()

    def upload(self, batch: ReadBatch, packed=None) -> DeviceBatch:
        """Resident copy of a host batch; ``packed``: with the SEQ column in its 4-bit form (``pack_seq``), which the
        tabulation (plain, with ``--min-basequal`` — the mask is folded into the column here, ``MDX_SEQ_4BITQ`` —
        or with the rescaling fused in) then reads through the packed kernels."""
        hb = _host_batch(batch, self.default_packed if packed is None else packed)
        dev = MdxBatch()
        self._check(self._lib.mdx_batch_upload(self._ctx, ctypes.byref(hb), ctypes.byref(dev)))
        return DeviceBatch(self, dev, batch.n, int(batch.seq.shape[0]), int(batch.cigar.shape[0]))

    def bgzf_deflate(self, data):
        """``data`` (bytes-like, host) as BGZF members of 0xFF00 input bytes each, deflated on the device (include/mdx.h
        ``mdx_bgzf_deflate``) -> uint8 array; no end-of-file marker."""
        view = np.frombuffer(memoryview(data).cast("B"), np.uint8)
        n = int(view.shape[0])
        out = np.empty(n + (n // 0xFF00 + 1) * 64, np.uint8)      # (a member of stored pieces: 26 + 5 per piece more than its bytes)
        out_len = ctypes.c_int64(0)
        fn = self._lib.mdx_bgzf_deflate
        fn.restype = ctypes.c_int
        self._check(fn(self._ctx, ctypes.c_void_p(view.ctypes.data), ctypes.c_int64(n), ctypes.c_void_p(out.ctypes.data),
                       ctypes.c_int64(out.shape[0]), ctypes.byref(out_len)))
        return out[:out_len.value]

    def fold(self, dbatch):
        """--min-basequal folded into a device batch's own 4-bit SEQ column, once and in place (include/mdx.h
        ``mdx_batch_fold``): a ``DeviceBatch`` or an ``MdxBatch`` of device pointers; it is ``MDX_SEQ_4BITQ`` afterwards."""
        dev = dbatch.dev if isinstance(dbatch, DeviceBatch) else dbatch
        self._lib.mdx_batch_fold.restype = ctypes.c_int
        self._check(self._lib.mdx_batch_fold(self._ctx, ctypes.byref(dev)))

    def _set_record_base(self, base):
        # (context state: every entry point that launches sets it, so that a base given to one call does not shift the
        # record numbers of the next)
        if base != getattr(self, "_record_base", 0):
            self._check(self._lib.mdx_set_record_base(self._ctx, ctypes.c_int64(base)))
            self._record_base = base

    def tabulate(self, batch, sync=True, record_base=None, packed=None):
        """Accumulate one batch (host ``ReadBatch`` or resident ``DeviceBatch``).  A host batch is staged through the
        library's pinned buffers: when the call returns its columns may be released.  ``sync=False`` leaves copies and
        kernel in flight (the next host batch is copied meanwhile); a record the reference cannot process then
        surfaces at the next ``sync()`` / ``finish()`` with index ``record_base`` + its index within its batch.
        ``packed`` (host batches): hand the SEQ column over in its 4-bit form (half the bytes across PCIe)."""
        self._set_record_base(0 if record_base is None else int(record_base))
        if isinstance(batch, DeviceBatch):
            self._last_n_reads = int(batch.dev.n_reads)
            self._check(self._lib.mdx_tabulate_device(self._ctx, ctypes.byref(batch.dev)))
        else:
            self._last_n_reads = int(batch.n)
            hb = _host_batch(batch, self.default_packed if packed is None else packed)
            self._check(self._lib.mdx_tabulate_host(self._ctx, ctypes.byref(hb)))
            if sync:
                # a record the reference cannot process surfaces here, with its index within this batch
                self.sync()

    def tabulate_view(self, view, record_base=None):
        """An ``MdxBatch`` of device pointers (``sam.GpuBamStream.next_view``): enqueued, errors at ``sync``."""
        self._set_record_base(0 if record_base is None else int(record_base))
        self._last_n_reads = int(view.n_reads)
        self._check(self._lib.mdx_tabulate_device(self._ctx, ctypes.byref(view)))

    def tabulate_pointers(self, n_reads, n_cigar, n_bases, **ptrs):
        """Device pointers owned by the caller (e.g. torch tensors): zero-copy entry."""
        b = MdxBatch()
        b.n_reads, b.n_cigar, b.n_bases = n_reads, n_cigar, n_bases
        for k, v in ptrs.items():
            setattr(b, k, v)
        self._set_record_base(0)
        self._check(self._lib.mdx_tabulate_device(self._ctx, ctypes.byref(b)))

    def sync(self):
        bad = ctypes.c_int64(-1)
        rc = self._lib.mdx_sync(self._ctx, ctypes.byref(bad))
        if rc == L.MDX_ERR_BAD_READ:
            raise BadReadError(bad.value, self._lib.mdx_last_error(self._ctx).decode())
        self._check(rc)

    # ------------------------------------------------------------------ outputs
    def table_words(self):
        return int(self._lib.mdx_table_words(self._ctx))

    def finish_device(self, device_ptr):
        """Write the packed canonical tables to a device buffer (for RCCL all-reduce)."""
        self._check(self._lib.mdx_finish_device(self._ctx, ctypes.c_void_p(device_ptr)))

    # ------------------------------------------------------------------ cross-device reduction (RCCL in the ABI)
    @staticmethod
    def comm_unique_id() -> bytes:
        """Rendezvous id for ``comm_init`` (ncclGetUniqueId): rank 0 creates it, every rank receives a copy."""
        buf = (ctypes.c_uint8 * 128)()
        rc = load_library().mdx_comm_unique_id(buf)
        if rc != 0:
            raise MdxError(rc, "mdx_comm_unique_id: librccl.so.1 could not be loaded")
        return bytes(buf)

    def comm_init(self, unique_id: bytes, nranks: int, rank: int):
        """Join the communicator (collective).  Afterwards ``finish()`` returns the totals over all ranks."""
        buf = (ctypes.c_uint8 * 128).from_buffer_copy(unique_id)
        self._check(self._lib.mdx_comm_init(self._ctx, buf, ctypes.c_int32(nranks), ctypes.c_int32(rank)))

    def comm_adopt(self, rccl_comm: int, nranks: int, rank: int):
        """Use a communicator the caller owns (an ``ncclComm_t`` as an integer, e.g. torch's
        ``ProcessGroupNCCL._comm_ptr()``); it is not destroyed with the engine."""
        self._check(self._lib.mdx_comm_adopt(self._ctx, ctypes.c_void_p(rccl_comm), ctypes.c_int32(nranks), ctypes.c_int32(rank)))

    @property
    def comm_size(self):
        return int(self._lib.mdx_comm_size(self._ctx))

    def comm_count(self):
        """The ranks RCCL counts in the attached communicator (ncclCommCount); 0 without one."""
        n = int(self._lib.mdx_comm_count(self._ctx))
        if n < 0:
            self._check(n)
        return n

    def finish_allreduce(self, device_ptr):
        """finish_device + in-place ncclAllReduce(uint64, sum) on the context's stream (collective)."""
        self._check(self._lib.mdx_finish_allreduce(self._ctx, ctypes.c_void_p(device_ptr)))

    def unpack_tables(self, words: np.ndarray, lgd_over=None) -> TableSet:
        """Split a packed table block (host copy of ``finish_device`` output)."""
        from .tables import unpack_words
        return unpack_words(words, self.libraries, self.length, self.around, self.lgd_max, lgd_over)

    def finish(self) -> TableSet:
        """Synchronise and fetch the canonical tables (main.py:229-231 reads them next).  With a communicator
        attached (``comm_init``) the call is collective and returns the totals over all ranks."""
        if self.groups is not None:
            return self._finish_strata()
        return self._finish_block()

    def _finish_block(self):
        if not self.comm_size:
            self.sync()
        nlib, Ln, A = len(self.libraries), self.length, self.around
        mis = np.zeros((nlib, 2, 2, Ln, L.N_MIS_COLS), np.uint64)
        comp = np.zeros((nlib, 2, 2, Ln + A, 4), np.uint64)
        lgd = np.zeros((nlib, 2, 2, self.lgd_max), np.uint64)
        # (with a communicator the list holds every rank's entries: each rank is bounded by lgd_over_cap)
        cap = max(1, self.lgd_over_cap) * max(1, self.comm_size)
        over = np.zeros((cap, 4), np.int64)
        n_over = ctypes.c_int64(0)
        n_kept = ctypes.c_int64(0)
        rc = self._lib.mdx_finish(self._ctx, _ptr(mis), _ptr(comp), _ptr(lgd), _ptr(over),
                                  ctypes.c_int64(cap), ctypes.byref(n_over), ctypes.byref(n_kept))
        if rc == L.MDX_ERR_BAD_READ:
            self.sync()     # raises BadReadError with the record's index
        self._check(rc)
        return TableSet(self.libraries, Ln, A, mis, comp, lgd, over[:n_over.value].copy(),
                        n_kept.value)

    def _finish_strata(self):
        """The block of all strata and — summed on the device, ``mdx_finish_merged_host`` — the block of the libraries."""
        from .tables import StratifiedTables, unpack_words
        if self.strata_kind is None:
            raise ValueError("finish: set_strata has not been called")
        if self.comm_size:
            raise ValueError("finish of a stratified engine with a communicator attached: reduce the block "
                             "(finish_allreduce) and split it with tables.StratifiedTables.from_block")
        strata = self._finish_block()
        out = StratifiedTables.from_block(strata, self.base_libraries, self.groups, self.strata_kept())
        if self.pmd_strata:
            out.pmd_hist, out.pmd_unqualified = self.pmd_histogram(), self.pmd_unqualified()
        merged = np.zeros(int(self._lib.mdx_merged_words(self._ctx)), np.uint64)
        self._check(self._lib.mdx_finish_merged_host(self._ctx, _ptr(merged)))
        out.merged = unpack_words(merged, self.base_libraries, self.length, self.around, self.lgd_max, out.merged.lgd_over)
        return out

    def lgd_overflow_only(self):
        """Out-of-range fragment-length records of this context (used after an all-reduce)."""
        self.sync()
        cap = max(1, self.lgd_over_cap)
        over = np.zeros((cap, 4), np.int64)
        n_over = ctypes.c_int64(0)
        self._check(self._lib.mdx_finish(self._ctx, None, None, None, _ptr(over), ctypes.c_int64(cap),
                                         ctypes.byref(n_over), None))
        return over[:min(cap, n_over.value)].copy()

    def genome_composition(self, n_contig):
        """Per-contig A, C, G, T counts of the resident reference (seqtk.comp of the reference)."""
        counts = np.zeros((n_contig, 4), np.uint64)
        self._check(self._lib.mdx_genome_composition(self._ctx, _ptr(counts)))
        return counts

    def set_rescale_model(self, model):
        """``model``: mapdamage_amd.rescale.RescaleModel."""
        lut = np.ascontiguousarray(model.lut, dtype=np.uint8)
        term = np.ascontiguousarray(model.term, dtype=np.float64)
        self._check(self._lib.mdx_rescale_set_model(self._ctx, _ptr(lut), _ptr(term),
                                                    ctypes.c_int32(model.len5p), ctypes.c_int32(model.len3p)))

    def rescale(self, batch: ReadBatch):
        """Rescaled qualities, raw MR sums (NaN = record unchanged) and routing status per record
        (mapdamage/rescale.py:285-365).  ``batch`` needs ``qual``, ``mtid`` and ``mpos``."""
        if batch.qual is None or batch.mtid is None or batch.mpos is None:
            raise ValueError("rescaling needs the qual, mtid and mpos columns")
        hb = _host_batch(batch)
        mtid = np.ascontiguousarray(batch.mtid, dtype=np.int32)
        mpos = np.ascontiguousarray(batch.mpos, dtype=np.int32)
        qual_out = np.zeros_like(batch.qual)
        mr = np.zeros(batch.n, np.float64)
        status = np.zeros(batch.n, np.uint8)
        rc = self._lib.mdx_rescale_host(self._ctx, ctypes.byref(hb), _ptr(mtid), _ptr(mpos), _ptr(qual_out),
                                        _ptr(mr), _ptr(status))
        if rc == L.MDX_ERR_BAD_READ:
            self.sync()     # raises BadReadError with the record's index within the batch
        self._check(rc)
        return qual_out, mr, status

    def rescale_device(self, dbatch, d_mtid, d_mpos, d_qual_out, d_mr, d_status, with_tables=False):
        """Rescale a resident batch (``DeviceBatch`` with qualities; the other arguments are device pointers as
        integers); ``with_tables``: count the batch into the tables in the same call (BASELINE configs[4])."""
        fn = self._lib.mdx_tabulate_rescale_device if with_tables else self._lib.mdx_rescale_device
        self._set_record_base(0)
        self._check(fn(self._ctx, ctypes.byref(dbatch.dev), ctypes.c_void_p(d_mtid), ctypes.c_void_p(d_mpos),
                       ctypes.c_void_p(d_qual_out), ctypes.c_void_p(d_mr), ctypes.c_void_p(d_status)))

    def rescale_patches(self, dbatch, d_mtid, d_mpos, d_patch, patch_cap, n_parts, d_n_patch, d_mr, d_status, with_tables=False):
        """``rescale_device`` with the rescaled bytes as a list (include/mdx.h ``mdx_*_patches_device``) in ``n_parts`` parts
        (a power of two): ``d_patch`` a device buffer of ``n_parts * patch_cap`` uint64 entries (byte index | new Phred <<
        32), ``d_n_patch`` ``n_parts`` device uint64 that receive the entries of each part."""
        fn = self._lib.mdx_tabulate_rescale_patches_device if with_tables else self._lib.mdx_rescale_patches_device
        fn.restype = ctypes.c_int
        dev = dbatch.dev if isinstance(dbatch, DeviceBatch) else dbatch
        self._set_record_base(0)
        self._check(fn(self._ctx, ctypes.byref(dev), ctypes.c_void_p(d_mtid), ctypes.c_void_p(d_mpos), ctypes.c_void_p(d_patch),
                       ctypes.c_int64(patch_cap), ctypes.c_int32(n_parts), ctypes.c_void_p(d_n_patch), ctypes.c_void_p(d_mr),
                       ctypes.c_void_p(d_status)))

    def rescale_expand(self, dbatch, d_patch, patch_cap, n_parts, d_n_patch, d_qual_out):
        """The batch's quality column with a patch list applied, into ``d_qual_out`` (device pointers)."""
        dev = dbatch.dev if isinstance(dbatch, DeviceBatch) else dbatch
        self._lib.mdx_rescale_expand_device.restype = ctypes.c_int
        self._check(self._lib.mdx_rescale_expand_device(self._ctx, ctypes.byref(dev), ctypes.c_void_p(d_patch), ctypes.c_int64(patch_cap),
                                                        ctypes.c_int32(n_parts), ctypes.c_void_p(d_n_patch), ctypes.c_void_p(d_qual_out)))

    def fused_launches(self):
        """Calls of rescale_device(with_tables=True) so far that ran as one fused launch."""
        return int(self._lib.mdx_fused_launches(self._ctx))

    def packed_launches(self):
        """Kernel launches so far that ran as the packed kernel (4-bit SEQ column and reference)."""
        return int(self._lib.mdx_packed_launches(self._ctx))

    def geo_spec_launches(self):
        """... and those of them that ran the packed kernel compiled for the default geometry (--length 70 --around 10, one
        library, no --min-basequal; ``MDX_NO_GEO_SPEC=1`` in the environment: none)."""
        return int(self._lib.mdx_geo_spec_launches(self._ctx))

    def libsorts(self):
        """Calls so far that bucketed their batch by library inside the launch (several libraries, a batch that did not
        bring the sorted columns: ``upload`` does)."""
        return int(self._lib.mdx_libsorts(self._ctx))

    def last_launch_geometry(self):
        """The context's last tabulation launch (``mdx_last_launch_geometry``): blocks of the grid, wavefronts per block, tiles
        of the call's whole batch (a launch over several libraries hands out its own libraries' share of them), pools of blocks
        that share a tile counter.  ``MDX_TEST_CUS=n`` in the environment when the engine is
        made sizes its launches as on a device of ``n`` compute units (tests: many tiles per wavefront of a small batch)."""
        out = np.zeros(4, np.int32)
        self._check(self._lib.mdx_last_launch_geometry(self._ctx, _ptr(out)))
        return dict(zip(("grid", "waves_per_block", "tiles", "pools"), (int(x) for x in out)))

    def rescale_timing_read(self):
        n = ctypes.c_int64(0)
        ms = ctypes.c_double(0)
        self._check(self._lib.mdx_rescale_timing_read(self._ctx, ctypes.byref(n), ctypes.byref(ms)))
        return n.value, ms.value

    def rescale_summary(self):
        """Integer content of the reference's ``subs`` dictionary (rescale.py:82-143) accumulated since
        set_rescale_model; mapdamage_amd.rescale.RescaleSummary turns it into the log lines."""
        n = int(self._lib.mdx_rescale_summary_words(self._ctx))
        words = np.zeros(n, np.uint64)
        self._check(self._lib.mdx_rescale_summary(self._ctx, _ptr(words)))
        return words

    def reset(self):
        self._check(self._lib.mdx_reset(self._ctx))

    # ------------------------------------------------------------------ timing
    def timing(self, enable=True):
        self._check(self._lib.mdx_timing_enable(self._ctx, 1 if enable else 0))

    def timing_read(self):
        n = ctypes.c_int64(0)
        ms = ctypes.c_double(0)
        self._check(self._lib.mdx_timing_read(self._ctx, ctypes.byref(n), ctypes.byref(ms)))
        return n.value, ms.value
