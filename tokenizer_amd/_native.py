"""ctypes binding of libtkz (include/tkz.h).  The library is the in-tree HIP build
(tokenizer_amd/lib/libtkz.so, produced by tokenizer_amd/csrc/Makefile or __graft_entry__.build()).
There is no fallback: if the library or a HIP device is missing, construction raises."""
import ctypes as C
import os

import numpy as np

_HERE = os.path.dirname(os.path.abspath(__file__))
# ($TKZ_LIBTKZ: development only -- e.g. the `make DEVPROF=1 OUT=../lib_dev` build with per-stage cycle counters)
DEFAULT_LIB = os.environ.get("TKZ_LIBTKZ") or os.path.join(_HERE, "lib", "libtkz.so")

OK = 0
E_FORMAT, E_DUP_RANK, E_KEY_NOT_FOUND, E_CAPACITY, E_INVALID_UTF8, E_ARG, E_UNSUPPORTED, E_DEVICE, E_NO_DEVICE, E_OUT_OF_MEMORY = range(-1, -11, -1)
ENGINE_DOTNET, ENGINE_ECMASCRIPT = 0, 1
P1, CL100K, O200K, O200K_DOTNET = 1, 2, 3, 4   # O200K: ECMAScript engine (TS reference); O200K_DOTNET: the same string through .NET Regex
OPT_PRETOK_SEQUENTIAL = 1
OPT_PIECE_MEMO = 2
OPT_PIECE_STATS = 3
OPT_PROMOTE_MIN_BYTES, OPT_PROMOTE_CAP = 5, 6
OPT_CASE_EQUIVALENCE = 7    # cl100k's (?i:...) with .NET >= 7's case-equivalence tables ('ſ is 's)
TRIM_SUFFIX, TRIM_PREFIX = 0, 1   # tkz_trim_side
PAD_RIGHT, PAD_LEFT = 0, 1         # tkz_pad_side
BUCKET_ASCENDING, BUCKET_DESCENDING = 0, 1   # tkz_bucket_order
TRUNC_LONGEST_FIRST, TRUNC_ONLY_FIRST, TRUNC_ONLY_SECOND = 0, 1, 2   # tkz_pair_truncation
NO_ROW_CAP = (1 << 31) - 1                    # bucket_rows of the budgeted entries: no cap on the rows of a bucket
OPT_LATENCY_BYTES = 8       # batches of at most this many bytes merge long missed pieces a wavefront each (tkz.h)
OPT_ADAPT = 9               # 1 (default): the encoder learns again when the text has drifted; small batches add up to a learning window (tkz.h)
OPT_PROMOTE = 4        # 0 / 1: automatic promotion of hot memo entries into the key tables off / on; 2: promote now; 3: drop the promotions
K_NAMES = ["k_docmark", "k_pretok", "k_probe", "k_scan", "k_place", "k_docoffs", "k_merge_long_group", "k_merge_short"]


class TkzError(Exception):
    """A non-OK tkz_status.  `.code` is the status; subclasses mirror the reference's exception types."""

    def __init__(self, code, msg):
        super().__init__("tkz status %d: %s" % (code, msg))
        self.code = code


class FormatError(TkzError):          # InvalidOperationException(FormatException)  TikTokenizer.cs:114-136
    pass


class DuplicateRankError(TkzError):   # ArgumentException                            TikTokenizer.cs:82-87
    pass


class KeyNotFoundError(TkzError, KeyError):   # KeyNotFoundException                 BytePairEncoder.cs:17,73
    pass


class UnsupportedError(TkzError, NotImplementedError):   # NotImplementedException   TokenizerBuilder.cs:179
    pass


_EXC = {E_FORMAT: FormatError, E_DUP_RANK: DuplicateRankError, E_KEY_NOT_FOUND: KeyNotFoundError, E_UNSUPPORTED: UnsupportedError}


class Library:
    def __init__(self, path=None):
        path = path or DEFAULT_LIB
        if not os.path.exists(path):
            raise RuntimeError("libtkz not built: %s is missing (run `python -c 'import __graft_entry__ as g; g.build()'` "
                               "or `make -C tokenizer_amd/csrc`); there is no CPU fallback" % path)
        self.path = path
        # PyTorch wheels bundle their own HIP runtime.  If torch is going to be used in this process (device
        # buffers, streams, torch.distributed) it has to initialise first, so that libtkz binds to the same
        # runtime instance; two runtimes in one process leave the second without a GPU.
        if os.path.basename(path) == "libtkz.so":
            try:
                import torch
                if torch.cuda.is_available():
                    torch.cuda.init()
            except ImportError:
                pass
        L = self.L = C.CDLL(path)
        vp, i64, i32, sz = C.c_void_p, C.c_int64, C.c_int32, C.c_size_t
        pv = C.POINTER(C.c_void_p)
        pi64 = C.POINTER(C.c_int64)
        L.tkz_last_error.restype = C.c_char_p
        L.tkz_vocab_from_tiktoken.argtypes = [vp, sz, pv]
        L.tkz_vocab_destroy.argtypes = [vp]
        L.tkz_vocab_destroy.restype = None
        L.tkz_vocab_size.argtypes = [vp]
        L.tkz_vocab_size.restype = i64
        L.tkz_vocab_max_key_len.argtypes = [vp]
        L.tkz_vocab_pair_table_entries.argtypes = [vp]
        L.tkz_vocab_pair_table_entries.restype = i64
        L.tkz_encoder_memo_slots.argtypes = [vp]
        L.tkz_encoder_memo_slots.restype = i64
        L.tkz_encoder_memo_ways.argtypes = [vp]
        L.tkz_encoder_small_path_calls.argtypes = [vp, pi64, pi64]
        L.tkz_encoder_small_path_calls.restype = None
        L.tkz_encoder_small_path_phases.argtypes = [vp, vp]
        L.tkz_encoder_memo_bucket.argtypes = [vp, vp, i32]
        L.tkz_encoder_memo_bucket.restype = i64
        L.tkz_unicode_classes.argtypes = [C.c_uint32, C.c_int32, vp]
        L.tkz_unicode_classes.restype = None
        L.tkz_encoder_unicode_classes.argtypes = [vp, C.c_uint32, C.c_int32, vp]
        L.tkz_encoder_set_unicode_classes.argtypes = [vp, vp, i64]
        L.tkz_encoder_pretok_leftovers.argtypes = [vp, pi64, pi64]
        L.tkz_encoder_pretok_leftovers.restype = None
        L.tkz_vocab_table_bytes.argtypes = [vp, C.c_int32]
        L.tkz_vocab_table_bytes.restype = i64
        L.tkz_vocab_rank.argtypes = [vp, vp, i32]
        L.tkz_pattern_from_regex.argtypes = [C.c_char_p, C.POINTER(i32)]
        L.tkz_pattern_from_regex_engine.argtypes = [C.c_char_p, i32, C.POINTER(i32)]
        L.tkz_encoder_create.argtypes = [vp, i32, i32, pv]
        L.tkz_encoder_destroy.argtypes = [vp]
        L.tkz_encoder_destroy.restype = None
        L.tkz_encoder_device.argtypes = [vp]
        L.tkz_encode_batch_utf8.argtypes = [vp, vp, vp, i64, vp, i64, vp, pi64]
        L.tkz_host_alloc.argtypes = [C.c_size_t, pv]
        L.tkz_host_free.argtypes = [vp]
        L.tkz_host_free.restype = None
        L.tkz_encode_batch_device.argtypes = [vp, vp, vp, i64, i64, vp, i64, vp, vp, pi64]
        L.tkz_encode_batch_device_begin.argtypes = [vp, vp, vp, i64, i64, vp, i64, vp, vp, C.POINTER(vp)]
        L.tkz_encode_batch_device_end.argtypes = [vp, pi64]
        L.tkz_encode_batch_device_begin_counts.argtypes = [vp, vp, vp, i64, i64, vp, i64, vp, vp, vp, C.POINTER(vp)]
        L.tkz_pending_counts_device.argtypes = [vp]
        L.tkz_pending_counts_device.restype = vp
        L.tkz_encode_batch_utf16.argtypes = [vp, vp, vp, i64, vp, i64, vp, pi64]
        L.tkz_encode_utf8.argtypes = [vp, vp, i64, vp, i64, pi64]
        L.tkz_encode_utf16.argtypes = [vp, vp, i64, vp, i64, pi64]
        L.tkz_encode_special_utf8.argtypes = [vp, vp, i64, vp, i32, vp, i64, pi64]
        L.tkz_encode_special_utf16.argtypes = [vp, vp, i64, vp, i32, vp, i64, pi64]
        L.tkz_encode_trim_utf8.argtypes = [vp, vp, i64, vp, i32, i32, i64, vp, i64, pi64, pi64, pi64]
        L.tkz_encode_trim_utf16.argtypes = [vp, vp, i64, vp, i32, i32, i64, vp, i64, pi64, pi64]
        L.tkz_pretokenize_utf8.argtypes = [vp, vp, vp, i64, vp]
        L.tkz_encode_pieces.argtypes = [vp, vp, vp, i64, vp, i64, vp, pi64]
        L.tkz_encode_batch_pieces_utf8.argtypes = [vp, vp, vp, i64, vp, i64, vp, vp, vp, i64, pi64, pi64]
        L.tkz_encoder_set_option.argtypes = [vp, i32, i64]
        L.tkz_encoder_piece_stats.argtypes = [vp, vp, i32]
        L.tkz_encoder_adapt_stats.argtypes = [vp, vp]
        L.tkz_encoder_reserve.argtypes = [vp, i64, i64]
        L.tkz_encoder_set_profiling.argtypes = [vp, i32]
        L.tkz_encoder_kernel_ms.argtypes = [vp, vp, vp, i32]
        L.tkz_encoder_workspace_bytes.argtypes = [vp]
        L.tkz_encoder_workspace_bytes.restype = i64
        L.tkz_encoder_side_by_side_batches.argtypes = [vp]
        L.tkz_encoder_side_by_side_batches.restype = i64
        L.tkz_encoder_engine_downloads.argtypes = [vp]
        L.tkz_encoder_engine_downloads.restype = i64
        L.tkz_kernel_name.argtypes = [i32]
        L.tkz_kernel_name.restype = C.c_char_p
        L.tkz_corpus_generate_device.argtypes = [i32, i32, C.c_uint64, i64, i64, i32, i32, vp, vp, i64, vp, pi64]
        L.tkz_corpus_generate_doc_host.argtypes = [i32, C.c_uint64, i64, i32, i32, vp, i64]
        L.tkz_corpus_generate_doc_host.restype = i64
        L.tkz_shard_range.argtypes = [i64, i32, i32, pi64, pi64]
        L.tkz_shard_range.restype = None
        L.tkz_shard_bases.argtypes = [vp, i32, i32, vp, vp]
        L.tkz_encoder_counts_device.argtypes = [vp]
        L.tkz_encoder_counts_device.restype = vp
        L.tkz_encoder_set_special_tokens.argtypes = [vp, vp, vp, vp, i32]
        L.tkz_encode_batch_special_device.argtypes = [vp, vp, vp, i64, i64, vp, i32, vp, i64, vp, vp, pi64]
        L.tkz_encode_batch_special_utf8.argtypes = [vp, vp, vp, i64, vp, i32, vp, i64, vp, pi64]
        L.tkz_encode_batch_trim_device.argtypes = [vp, vp, vp, i64, i64, vp, i32, i32, i64, vp, vp, i64, vp, vp, vp, vp, pi64]
        L.tkz_encode_batch_trim_utf8.argtypes = [vp, vp, vp, i64, vp, i32, i32, i64, vp, vp, i64, vp, vp, vp, pi64]
        L.tkz_encode_batch_special_utf16.argtypes = [vp, vp, vp, i64, vp, i32, vp, i64, vp, pi64]
        L.tkz_encode_batch_trim_utf16.argtypes = [vp, vp, vp, i64, vp, i32, i32, i64, vp, vp, i64, vp, vp, pi64]
        L.tkz_encoder_special_stats.argtypes = [vp, pi64, pi64]
        L.tkz_encoder_special_stats.restype = None
        L.tkz_decode_batch_device.argtypes = [vp, vp, vp, i64, i64, vp, i64, vp, vp, pi64]
        L.tkz_decode_batch.argtypes = [vp, vp, vp, i64, vp, i64, vp, pi64]
        L.tkz_decode_batch_utf16_device.argtypes = [vp, vp, vp, i64, i64, vp, i64, vp, vp, pi64]
        L.tkz_decode_batch_utf16.argtypes = [vp, vp, vp, i64, vp, i64, vp, pi64]
        L.tkz_decode_utf8.argtypes = [vp, vp, i64, vp, i64, pi64]
        L.tkz_decode_utf16.argtypes = [vp, vp, i64, vp, i64, pi64]
        L.tkz_encoder_small_decode_calls.argtypes = [vp, pi64, pi64]
        L.tkz_encoder_small_decode_calls.restype = None
        L.tkz_encoder_small_decode_phases.argtypes = [vp, vp]
        L.tkz_count_batch_device.argtypes = [vp, vp, vp, i64, i64, vp, i32, vp, vp, pi64]
        L.tkz_count_batch_utf8.argtypes = [vp, vp, vp, i64, vp, i32, vp, pi64]
        L.tkz_count_batch_utf16.argtypes = [vp, vp, vp, i64, vp, i32, vp, pi64]
        L.tkz_count_utf8.argtypes = [vp, vp, i64, vp, i32, pi64]
        L.tkz_count_utf16.argtypes = [vp, vp, i64, vp, i32, pi64]
        L.tkz_encoder_count_calls.argtypes = [vp, pi64, pi64]
        L.tkz_encoder_count_calls.restype = None
        L.tkz_encode_batch_spans_device.argtypes = [vp, vp, vp, i64, i64, vp, i32, vp, i64, vp, vp, vp, vp, pi64]
        L.tkz_encode_batch_spans_utf8.argtypes = [vp, vp, vp, i64, vp, i32, vp, i64, vp, vp, vp, pi64]
        L.tkz_encode_batch_spans_utf16.argtypes = [vp, vp, vp, i64, vp, i32, vp, i64, vp, vp, pi64]
        L.tkz_encode_spans_utf8.argtypes = [vp, vp, i64, vp, i32, vp, i64, vp, vp, pi64]
        L.tkz_encode_spans_utf16.argtypes = [vp, vp, i64, vp, i32, vp, i64, vp, pi64]
        L.tkz_encoder_spans_calls.argtypes = [vp, pi64]
        L.tkz_encoder_spans_calls.restype = None
        L.tkz_encode_batch_chunks_device.argtypes = [vp, vp, vp, i64, i64, vp, i32, i64, vp, i64, vp, vp, vp, vp, vp, i64, vp, pi64, pi64]
        L.tkz_encode_batch_chunks_utf8.argtypes = [vp, vp, vp, i64, vp, i32, i64, vp, i64, vp, vp, vp, vp, vp, i64, pi64, pi64]
        L.tkz_encode_batch_chunks_utf16.argtypes = [vp, vp, vp, i64, vp, i32, i64, vp, i64, vp, vp, vp, vp, i64, pi64, pi64]
        L.tkz_encode_chunks_utf8.argtypes = [vp, vp, i64, vp, i32, i64, vp, i64, vp, vp, vp, i64, pi64, pi64]
        L.tkz_encode_chunks_utf16.argtypes = [vp, vp, i64, vp, i32, i64, vp, i64, vp, vp, i64, pi64, pi64]
        L.tkz_encoder_chunks_calls.argtypes = [vp, pi64]
        L.tkz_encoder_chunks_calls.restype = None
        L.tkz_encode_batch_chunks_overlap_device.argtypes = [vp, vp, vp, i64, i64, vp, i32, i64, i64, vp, i64, vp, vp, vp, vp, vp, vp, vp, vp, i64, vp, pi64, pi64]
        L.tkz_encode_batch_chunks_overlap_utf8.argtypes = [vp, vp, vp, i64, vp, i32, i64, i64, vp, i64, vp, vp, vp, vp, vp, vp, vp, vp, i64, pi64, pi64]
        L.tkz_encode_batch_chunks_overlap_utf16.argtypes = [vp, vp, vp, i64, vp, i32, i64, i64, vp, i64, vp, vp, vp, vp, vp, vp, i64, pi64, pi64]
        L.tkz_encode_chunks_overlap_utf8.argtypes = [vp, vp, i64, vp, i32, i64, i64, vp, i64, vp, vp, vp, vp, vp, vp, i64, pi64, pi64]
        L.tkz_encode_chunks_overlap_utf16.argtypes = [vp, vp, i64, vp, i32, i64, i64, vp, i64, vp, vp, vp, vp, i64, pi64, pi64]
        L.tkz_encoder_chunks_overlap_calls.argtypes = [vp, pi64]
        L.tkz_encoder_chunks_overlap_calls.restype = None
        L.tkz_encode_batch_packed_device.argtypes = [vp, vp, vp, i64, i64, vp, i32, i32, i32, i64, i32, vp, i64, vp, vp, vp, i64, vp, pi64, pi64, pi64]
        L.tkz_encode_batch_packed_utf8.argtypes = [vp, vp, vp, i64, vp, i32, i32, i32, i64, i32, vp, i64, vp, vp, vp, i64, pi64, pi64, pi64]
        L.tkz_encode_batch_packed_utf16.argtypes = [vp, vp, vp, i64, vp, i32, i32, i32, i64, i32, vp, i64, vp, vp, vp, i64, pi64, pi64, pi64]
        L.tkz_encoder_packed_calls.argtypes = [vp, pi64]
        L.tkz_encoder_packed_calls.restype = None
        L.tkz_encode_batch_padded_device.argtypes = [vp, vp, vp, i64, i64, vp, i32, i32, i32, i64, i32, i32, i32, i64, vp, i64, vp, vp, vp, vp, vp, pi64, pi64, pi64]
        L.tkz_encode_batch_padded_utf8.argtypes = [vp, vp, vp, i64, vp, i32, i32, i32, i64, i32, i32, i32, i64, vp, i64, vp, vp, vp, vp, pi64, pi64, pi64]
        L.tkz_encode_batch_padded_utf16.argtypes = [vp, vp, vp, i64, vp, i32, i32, i32, i64, i32, i32, i32, i64, vp, i64, vp, vp, vp, vp, pi64, pi64, pi64]
        L.tkz_encoder_padded_calls.argtypes = [vp, pi64]
        L.tkz_encoder_padded_calls.restype = None
        L.tkz_encode_batch_bucketed_device.argtypes = [vp, vp, vp, i64, i64, vp, i32, i32, i32, i64, i32, i32, i32, i64, i64, i32, vp, i64, vp, vp, vp, vp, vp, vp, vp, vp, vp,
                                                       pi64, pi64, pi64]
        L.tkz_encode_batch_bucketed_utf8.argtypes = [vp, vp, vp, i64, vp, i32, i32, i32, i64, i32, i32, i32, i64, i64, i32, vp, i64, vp, vp, vp, vp, vp, vp, vp, vp, pi64, pi64, pi64]
        L.tkz_encode_batch_bucketed_utf16.argtypes = [vp, vp, vp, i64, vp, i32, i32, i32, i64, i32, i32, i32, i64, i64, i32, vp, i64, vp, vp, vp, vp, vp, vp, vp, vp, pi64, pi64, pi64]
        L.tkz_encoder_bucketed_calls.argtypes = [vp, pi64]
        L.tkz_encoder_bucketed_calls.restype = None
        L.tkz_encode_batch_budgeted_device.argtypes = [vp, vp, vp, i64, i64, vp, i32, i32, i32, i64, i32, i32, i32, i64, i64, i64, i32, vp, i64, vp, vp, vp, vp, vp, vp, vp, vp,
                                                       vp, i64, vp, pi64, pi64, pi64, pi64]
        L.tkz_encode_batch_budgeted_utf8.argtypes = [vp, vp, vp, i64, vp, i32, i32, i32, i64, i32, i32, i32, i64, i64, i64, i32, vp, i64, vp, vp, vp, vp, vp, vp, vp, vp, vp, i64,
                                                     pi64, pi64, pi64, pi64]
        L.tkz_encode_batch_budgeted_utf16.argtypes = list(L.tkz_encode_batch_budgeted_utf8.argtypes)
        L.tkz_encoder_budgeted_calls.argtypes = [vp, pi64]
        L.tkz_encoder_budgeted_calls.restype = None
        L.tkz_encode_batch_pairs_device.argtypes = [vp, vp, vp, i64, i64, vp, i32, i32, i32, i32, i32, i64, i32, i32, i32, i32, i64, vp, i64, vp, vp, vp, vp, vp, vp, vp,
                                                    pi64, pi64, pi64]
        L.tkz_encode_batch_pairs_utf8.argtypes = [vp, vp, vp, i64, vp, i32, i32, i32, i32, i32, i64, i32, i32, i32, i32, i64, vp, i64, vp, vp, vp, vp, vp, vp, pi64, pi64, pi64]
        L.tkz_encode_batch_pairs_utf16.argtypes = list(L.tkz_encode_batch_pairs_utf8.argtypes)
        L.tkz_encoder_pairs_calls.argtypes = [vp, pi64]
        L.tkz_encoder_pairs_calls.restype = None
        L.tkz_shard_write.argtypes = [C.c_char_p, vp, i64, vp, i64, i64, i64]
        L.tkz_shard_write_device.argtypes = [C.c_char_p, i32, vp, i64, vp, i64, i64, i64]
        L.tkz_shard_read_header.argtypes = [C.c_char_p, pi64, pi64, pi64, pi64]
        self.has_comm = hasattr(L, "tkz_comm_create")      # (the CPU emulator build of the tests has no communicator)
        if self.has_comm:
            L.tkz_comm_unique_id.argtypes = [vp]
            L.tkz_comm_create.argtypes = [vp, i32, i32, i32, pv]
            L.tkz_comm_destroy.argtypes = [vp]
            L.tkz_comm_destroy.restype = None
            L.tkz_comm_world.argtypes = [vp]
            L.tkz_comm_rank.argtypes = [vp]
            L.tkz_comm_backend.argtypes = [vp]
            L.tkz_comm_backend.restype = C.c_char_p
            L.tkz_comm_allgather_counts_device.argtypes = [vp, vp, vp, vp]
            L.tkz_comm_allgather_counts.argtypes = [vp, i64, i64, i64, vp]

    def check(self, status):
        if status != OK:
            msg = (self.L.tkz_last_error() or b"").decode("utf-8", "replace")
            raise _EXC.get(status, TkzError)(status, msg)


_default = None


def default_library():
    global _default
    if _default is None:
        _default = Library()
    return _default


def _ptr(a):
    return a.ctypes.data if a is not None else None


class Vocab:
    """LoadTikTokenBpe + Init's duplicate-rank check (TikTokenizer.cs:99-139, :74-91)."""

    def __init__(self, tiktoken_bytes: bytes, lib: Library = None):
        self.lib = lib or default_library()
        h = C.c_void_p()
        buf = (C.c_uint8 * max(1, len(tiktoken_bytes))).from_buffer_copy(tiktoken_bytes or b"\0")
        self.lib.check(self.lib.L.tkz_vocab_from_tiktoken(buf, len(tiktoken_bytes), C.byref(h)))
        self._h = h

    def __del__(self):
        if getattr(self, "_h", None):
            self.lib.L.tkz_vocab_destroy(self._h)
            self._h = None

    def __len__(self):
        return self.lib.L.tkz_vocab_size(self._h)

    @property
    def max_key_len(self):
        return self.lib.L.tkz_vocab_max_key_len(self._h)

    @property
    def pair_table_entries(self):
        return self.lib.L.tkz_vocab_pair_table_entries(self._h)

    def table_bytes(self):
        """Bytes of every device table image: {"short", "mid", "long", "pair", "direct", "total"}."""
        f = self.lib.L.tkz_vocab_table_bytes
        d = {k: int(f(self._h, i)) for i, k in enumerate(("short", "mid", "long", "pair", "direct"))}
        d["total"] = int(f(self._h, -1))
        return d

    def rank(self, key: bytes):
        buf = (C.c_uint8 * max(1, len(key))).from_buffer_copy(key or b"\0")
        return self.lib.L.tkz_vocab_rank(self._h, buf, len(key))


class Encoder:
    """The device encoder (tables in HBM + workspace)."""

    def __init__(self, vocab: Vocab, pattern: int, device: int = 0):
        self.lib = vocab.lib
        h = C.c_void_p()
        self.lib.check(self.lib.L.tkz_encoder_create(vocab._h, pattern, device, C.byref(h)))
        self._h = h
        self.pattern = pattern

    def close(self):
        if getattr(self, "_h", None):
            self.lib.L.tkz_encoder_destroy(self._h)
            self._h = None

    def __del__(self):
        self.close()

    def set_option(self, opt, value):
        self.lib.check(self.lib.L.tkz_encoder_set_option(self._h, opt, value))

    def set_unicode_classes(self, classes):
        """The host's Unicode classification (tkz_encoder_set_unicode_classes): uint8[65536] (code units) or uint8[1114112] (code points) of class
        codes 0..8, or None for the built-in Unicode 13.0 table."""
        if classes is None:
            self.lib.check(self.lib.L.tkz_encoder_set_unicode_classes(self._h, None, 0))
            return
        a = np.ascontiguousarray(classes, dtype=np.uint8)
        self.lib.check(self.lib.L.tkz_encoder_set_unicode_classes(self._h, a.ctypes.data, len(a)))

    def unicode_classes(self, first, n):
        """Classes of code points first .. first + n - 1 as the DEVICE's table has them (tkz_encoder_unicode_classes)."""
        out = np.zeros(n, np.uint8)
        self.lib.check(self.lib.L.tkz_encoder_unicode_classes(self._h, first, n, out.ctypes.data))
        return out

    def piece_stats(self, reset=False):
        """What the batch path met since the last reset, with OPT_PIECE_STATS on (tkz_encoder_piece_stats)."""
        out = np.zeros(8, np.int64)
        self.lib.check(self.lib.L.tkz_encoder_piece_stats(self._h, out.ctypes.data, 1 if reset else 0))
        pieces, sm, lm, gm, look, hit = (int(out[i]) for i in (1, 2, 3, 4, 5, 6))
        return {"batches": int(out[0]), "pieces": pieces, "short_misses": sm, "long_misses": lm, "giant_pieces": gm,
                "whole_piece_hit_rate": round(1.0 - (sm + lm + gm) / pieces, 5) if pieces else None,
                "memo_lookups": look, "memo_hits": hit, "memo_hit_rate": round(hit / look, 5) if look else None,
                "merged_short": look - hit if look else sm, "promoted_pieces_in_tables": int(out[7])}

    def reserve(self, max_bytes, max_docs):
        """The workspace of batches of up to max_bytes / max_docs, allocated now instead of inside the first batch call (tkz_encoder_reserve)."""
        self.lib.check(self.lib.L.tkz_encoder_reserve(self._h, int(max_bytes), int(max_docs)))

    def adapt_stats(self):
        """TKZ_OPT_ADAPT's bookkeeping (tkz_encoder_adapt_stats): promotions, re-learns, promoted pieces, the settled and the recent miss share."""
        out = np.zeros(8, np.int64)
        self.lib.check(self.lib.L.tkz_encoder_adapt_stats(self._h, out.ctypes.data))
        return {"promotions": int(out[0]), "relearns": int(out[1]), "promoted_pieces": int(out[2]), "retired_images": int(out[3]),
                "settled_miss_share": None if out[4] < 0 else out[4] / 1e6, "recent_miss_share": None if out[5] < 0 else out[5] / 1e6,
                "bytes_since_tables_changed": int(out[6]), "learning_window_bytes": int(out[7])}

    def set_profiling(self, on):
        self.lib.check(self.lib.L.tkz_encoder_set_profiling(self._h, 1 if on else 0))

    def kernel_ms(self, reset=False):
        ms = np.zeros(len(K_NAMES), np.float64)
        n = np.zeros(len(K_NAMES), np.int64)
        self.lib.check(self.lib.L.tkz_encoder_kernel_ms(self._h, ms.ctypes.data, n.ctypes.data, 1 if reset else 0))
        return {K_NAMES[i]: (float(ms[i]), int(n[i])) for i in range(len(K_NAMES))}

    @property
    def memo_slots(self):
        return int(self.lib.L.tkz_encoder_memo_slots(self._h))

    @property
    def memo_ways(self):
        return int(self.lib.L.tkz_encoder_memo_ways(self._h))

    def memo_bucket(self, piece: bytes):
        """Bucket of the piece memo a piece of 1..16 bytes uses (-1: none; pieces holding a zero byte never use the memo)."""
        return int(self.lib.L.tkz_encoder_memo_bucket(self._h, piece, len(piece)))

    def small_path_calls(self):
        """(calls that took the single-launch path for small batches, how many of those it handed back to the batch path)."""
        a, b = C.c_int64(0), C.c_int64(0)
        self.lib.L.tkz_encoder_small_path_calls(self._h, C.byref(a), C.byref(b))
        return a.value, b.value

    def small_path_phases(self):
        """Shader-clock stamps at the end of the phases of the last single-launch kernel (development)."""
        a = np.zeros(16, np.int64)
        n = self.lib.L.tkz_encoder_small_path_phases(self._h, a.ctypes.data)
        return a[:n].tolist()

    def small_decode_calls(self):
        """(single decode calls that took the launch of k_dec_small, how many of those it handed back to the batch path)."""
        a, b = C.c_int64(0), C.c_int64(0)
        self.lib.L.tkz_encoder_small_decode_calls(self._h, C.byref(a), C.byref(b))
        return a.value, b.value

    def small_decode_phases(self):
        """Shader-clock stamps at the end of the phases of the last k_dec_small (development)."""
        a = np.zeros(16, np.int64)
        n = self.lib.L.tkz_encoder_small_decode_phases(self._h, a.ctypes.data)
        return a[:n].tolist()

    def pretok_leftovers(self):
        """(blocks the o200k ASCII block scanner handed on, blocks the multi-byte block scanner handed on to the sequential matcher) of the last batch."""
        a, b = C.c_int64(0), C.c_int64(0)
        self.lib.L.tkz_encoder_pretok_leftovers(self._h, C.byref(a), C.byref(b))
        return a.value, b.value

    @property
    def workspace_bytes(self):
        return self.lib.L.tkz_encoder_workspace_bytes(self._h)

    @property
    def engine_downloads(self):
        """Copies of host-call results that left the device on a copy engine of their own (tkz_encoder_engine_downloads)."""
        return self.lib.L.tkz_encoder_engine_downloads(self._h)

    @property
    def side_by_side_batches(self):
        """Batches whose long-piece kernels ran beside k_merge_short on streams of their own (tkz_encoder_side_by_side_batches)."""
        return self.lib.L.tkz_encoder_side_by_side_batches(self._h)

    # -- host buffers --
    def encode_batch(self, data: np.ndarray, offsets: np.ndarray, out_cap=None, out=None):
        """EncodeBatch: (ids int32[total_tokens], out_offsets int64[n+1]).  `out` = (ids, out_offsets) arrays to fill
        (e.g. views of page-locked memory: the copies over PCIe then run at link speed instead of through a bounce buffer)."""
        data = np.ascontiguousarray(data, dtype=np.uint8)
        offsets = np.ascontiguousarray(offsets, dtype=np.int64)
        n = len(offsets) - 1
        cap = len(data) if out_cap is None else out_cap
        if out is not None:
            ids, ooff = out
            assert ids.dtype == np.int32 and ooff.dtype == np.int64 and ids.flags.c_contiguous and ooff.flags.c_contiguous
            assert len(ooff) >= n + 1
            cap = len(ids)
        else:
            ids = np.empty(max(1, cap), np.int32)
            ooff = np.empty(n + 1, np.int64)
        needed = C.c_int64(0)
        self.lib.check(self.lib.L.tkz_encode_batch_utf8(self._h, _ptr(data), _ptr(offsets), n, _ptr(ids), cap, _ptr(ooff), C.byref(needed)))
        return ids[:needed.value], ooff[:n + 1]

    def encode_batch_special(self, data: np.ndarray, offsets: np.ndarray, allowed, out_cap=None, out=None):
        """EncodeBatch as ITokenizer.Encode(text, allowedSpecial): the allowed special-token literals are cut out on the device.  allowed: indices into the
        literals registered by set_special_tokens (registration order).  Buffers as in encode_batch."""
        data = np.ascontiguousarray(data, dtype=np.uint8)
        offsets = np.ascontiguousarray(offsets, dtype=np.int64)
        allowed = np.ascontiguousarray(allowed, dtype=np.int32)
        n = len(offsets) - 1
        cap = len(data) if out_cap is None else out_cap
        if out is not None:
            ids, ooff = out
            assert ids.dtype == np.int32 and ooff.dtype == np.int64 and ids.flags.c_contiguous and ooff.flags.c_contiguous
            assert len(ooff) >= n + 1
            cap = len(ids)
        else:
            ids = np.empty(max(1, cap), np.int32)
            ooff = np.empty(n + 1, np.int64)
        needed = C.c_int64(0)
        self.lib.check(self.lib.L.tkz_encode_batch_special_utf8(self._h, _ptr(data), _ptr(offsets), n, _ptr(allowed) if len(allowed) else None, len(allowed),
                                                                _ptr(ids), cap, _ptr(ooff), C.byref(needed)))
        return ids[:needed.value], ooff[:n + 1]

    def encode_batch_special_device(self, d_bytes, d_offsets, n_docs, total_bytes, allowed, d_out_ids, out_cap, d_out_offsets, stream=0):
        allowed = np.ascontiguousarray(allowed, dtype=np.int32)
        tot = C.c_int64(0)
        self.lib.check(self.lib.L.tkz_encode_batch_special_device(self._h, d_bytes, d_offsets, n_docs, total_bytes, _ptr(allowed) if len(allowed) else None,
                                                                  len(allowed), d_out_ids, out_cap, d_out_offsets, stream or None, C.byref(tot)))
        return tot.value

    def encode_batch_trim(self, data: np.ndarray, offsets: np.ndarray, allowed_index, side, max_tokens, per_doc=None, out_cap=None):
        """EncodeTrimSuffix (side TRIM_SUFFIX) / EncodeTrimPrefix (TRIM_PREFIX) for a batch, cut on the device: (kept ids int32, offsets int64[n+1],
        cut_bytes int64[n], cut_units int64[n]) -- the byte and UTF-16 length of the kept (suffix) or dropped (prefix) text of every document.  allowed_index as in
        encode_batch_special; per_doc: a maximum per document (int64[n]) in place of max_tokens.  out_cap counts the kept ids."""
        data = np.ascontiguousarray(data, dtype=np.uint8)
        offsets = np.ascontiguousarray(offsets, dtype=np.int64)
        allowed = np.ascontiguousarray(allowed_index, dtype=np.int32)
        n = len(offsets) - 1
        if per_doc is not None:
            per_doc = np.ascontiguousarray(per_doc, dtype=np.int64)
            assert len(per_doc) == n
            bound = int(np.minimum(np.maximum(per_doc, 0), np.diff(offsets)).sum()) if n else 0
        else:
            bound = min(len(data), n * max(int(max_tokens), 0))
        cap = bound if out_cap is None else out_cap
        ids = np.empty(max(1, cap), np.int32)
        ooff = np.empty(n + 1, np.int64)
        cb, cu = np.zeros(max(1, n), np.int64), np.zeros(max(1, n), np.int64)
        needed = C.c_int64(0)
        try:
            self.lib.check(self.lib.L.tkz_encode_batch_trim_utf8(self._h, _ptr(data) if len(data) else None, _ptr(offsets), n, _ptr(allowed) if len(allowed) else None,
                                                                 len(allowed), int(side), int(max_tokens), _ptr(per_doc) if per_doc is not None and n else None,
                                                                 _ptr(ids), cap, _ptr(ooff), _ptr(cb), _ptr(cu), C.byref(needed)))
        except TkzError as ex:
            ex.needed = needed.value                          # (E_CAPACITY: the kept total)
            raise
        return ids[:needed.value], ooff, cb[:n], cu[:n]

    def encode_batch_trim_device(self, d_bytes, d_offsets, n_docs, total_bytes, allowed, side, max_tokens, d_max_tokens, d_out_ids, out_cap, d_out_offsets,
                                 d_cut_bytes=0, d_cut_units=0, stream=0):
        allowed = np.ascontiguousarray(allowed, dtype=np.int32)
        tot = C.c_int64(0)
        try:
            self.lib.check(self.lib.L.tkz_encode_batch_trim_device(self._h, d_bytes, d_offsets, n_docs, total_bytes, _ptr(allowed) if len(allowed) else None, len(allowed),
                                                                   int(side), int(max_tokens), d_max_tokens or None, d_out_ids or None, out_cap, d_out_offsets,
                                                                   d_cut_bytes or None, d_cut_units or None, stream or None, C.byref(tot)))
        except TkzError as ex:
            ex.needed = tot.value                             # (E_CAPACITY: the kept total)
            raise
        return tot.value

    def special_stats(self):
        """(calls that took the device special path, special-token literals they turned into ids)"""
        b, l = C.c_int64(0), C.c_int64(0)
        self.lib.L.tkz_encoder_special_stats(self._h, C.byref(b), C.byref(l))
        return b.value, l.value

    def encode_batch_utf16(self, units: np.ndarray, offsets: np.ndarray, out=None):
        """EncodeBatch on UTF-16 code units (uint16[total], offsets int64[n+1] in units); transcoded on the device.
        `out` = (ids, out_offsets) arrays to fill, as in encode_batch."""
        units = np.ascontiguousarray(units, dtype=np.uint16)
        offsets = np.ascontiguousarray(offsets, dtype=np.int64)
        n = len(offsets) - 1
        if out is not None:
            ids, ooff = out
            assert ids.dtype == np.int32 and ooff.dtype == np.int64 and ids.flags.c_contiguous and ooff.flags.c_contiguous and len(ooff) >= n + 1
            cap = len(ids)
        else:
            cap = max(1, 3 * len(units))
            ids = np.empty(cap, np.int32)
            ooff = np.empty(n + 1, np.int64)
        needed = C.c_int64(0)
        buf = units if len(units) else np.zeros(1, np.uint16)
        self.lib.check(self.lib.L.tkz_encode_batch_utf16(self._h, _ptr(buf), _ptr(offsets), n, _ptr(ids), cap, _ptr(ooff), C.byref(needed)))
        return ids[:needed.value], ooff[:n + 1]

    def encode_batch_special_utf16(self, units: np.ndarray, offsets: np.ndarray, allowed_index, out=None, out_cap=None):
        """ITokenizer.Encode(text, allowedSpecial) for a batch of UTF-16 documents (uint16[total], offsets int64[n+1] in units): transcoded on the device, the
        literals searched as .NET searches the string (a lone surrogate is not U+FFFD).  allowed_index as in encode_batch_special.  (ids, offsets)."""
        units = np.ascontiguousarray(units, dtype=np.uint16)
        offsets = np.ascontiguousarray(offsets, dtype=np.int64)
        allowed = np.ascontiguousarray(allowed_index, dtype=np.int32)
        n = len(offsets) - 1
        if out is not None:
            ids, ooff = out
            assert ids.dtype == np.int32 and ooff.dtype == np.int64 and ids.flags.c_contiguous and ooff.flags.c_contiguous and len(ooff) >= n + 1
            cap = len(ids)
        else:
            cap = 3 * len(units) if out_cap is None else out_cap
            ids = np.empty(max(1, cap), np.int32)
            ooff = np.empty(n + 1, np.int64)
        needed = C.c_int64(0)
        buf = units if len(units) else np.zeros(1, np.uint16)
        try:
            self.lib.check(self.lib.L.tkz_encode_batch_special_utf16(self._h, _ptr(buf), _ptr(offsets), n, _ptr(allowed) if len(allowed) else None, len(allowed),
                                                                     _ptr(ids), cap, _ptr(ooff), C.byref(needed)))
        except TkzError as ex:
            ex.needed = needed.value                          # (E_CAPACITY: the total)
            raise
        return ids[:needed.value], ooff[:n + 1]

    def encode_batch_trim_utf16(self, units: np.ndarray, offsets: np.ndarray, allowed_index, side, max_tokens, per_doc=None, out_cap=None):
        """encode_batch_trim for UTF-16 documents: (kept ids int32, offsets int64[n+1], cut_units int64[n]) -- the kept (suffix) or dropped (prefix) text of
        document d is its first cut_units[d] code units."""
        units = np.ascontiguousarray(units, dtype=np.uint16)
        offsets = np.ascontiguousarray(offsets, dtype=np.int64)
        allowed = np.ascontiguousarray(allowed_index, dtype=np.int32)
        n = len(offsets) - 1
        if per_doc is not None:
            per_doc = np.ascontiguousarray(per_doc, dtype=np.int64)
            assert len(per_doc) == n
            bound = int(np.minimum(np.maximum(per_doc, 0), 3 * np.diff(offsets)).sum()) if n else 0
        else:
            bound = min(3 * len(units), n * max(int(max_tokens), 0))
        cap = bound if out_cap is None else out_cap
        ids = np.empty(max(1, cap), np.int32)
        ooff = np.empty(n + 1, np.int64)
        cu = np.zeros(max(1, n), np.int64)
        needed = C.c_int64(0)
        buf = units if len(units) else np.zeros(1, np.uint16)
        try:
            self.lib.check(self.lib.L.tkz_encode_batch_trim_utf16(self._h, _ptr(buf), _ptr(offsets), n, _ptr(allowed) if len(allowed) else None, len(allowed),
                                                                  int(side), int(max_tokens), _ptr(per_doc) if per_doc is not None and n else None,
                                                                  _ptr(ids), cap, _ptr(ooff), _ptr(cu), C.byref(needed)))
        except TkzError as ex:
            ex.needed = needed.value                          # (E_CAPACITY: the kept total)
            raise
        return ids[:needed.value], ooff, cu[:n]

    def encode_pieces(self, data: np.ndarray, offsets: np.ndarray):
        data = np.ascontiguousarray(data, dtype=np.uint8)
        offsets = np.ascontiguousarray(offsets, dtype=np.int64)
        n = len(offsets) - 1
        ids = np.empty(max(1, len(data)), np.int32)
        ooff = np.empty(n + 1, np.int64)
        needed = C.c_int64(0)
        self.lib.check(self.lib.L.tkz_encode_pieces(self._h, _ptr(data), _ptr(offsets), n, _ptr(ids), len(data), _ptr(ooff), C.byref(needed)))
        return ids[:needed.value], ooff

    def encode_batch_pieces(self, data: np.ndarray, offsets: np.ndarray):
        """EncodeBatch with piece granularity: (ids, doc_piece_offsets[n+1], piece_byte_offsets[np+1], piece_token_offsets[np+1])."""
        data = np.ascontiguousarray(data, dtype=np.uint8)
        offsets = np.ascontiguousarray(offsets, dtype=np.int64)
        n = len(offsets) - 1
        cap = max(1, len(data))
        ids = np.empty(cap, np.int32)
        dpo = np.empty(n + 1, np.int64)
        pbo = np.empty(cap + 1, np.int64)
        pto = np.empty(cap + 1, np.int64)
        npieces, needed = C.c_int64(0), C.c_int64(0)
        self.lib.check(self.lib.L.tkz_encode_batch_pieces_utf8(self._h, _ptr(data), _ptr(offsets), n, _ptr(ids), cap, _ptr(dpo), _ptr(pbo),
                                                               _ptr(pto), cap, C.byref(npieces), C.byref(needed)))
        k = npieces.value
        return ids[:needed.value], dpo, pbo[:k + 1], pto[:k + 1]

    def pretokenize(self, data: np.ndarray, offsets: np.ndarray):
        """Piece-start bitmap as a bool array of len(data) + 1 (the last entry is the sentinel)."""
        data = np.ascontiguousarray(data, dtype=np.uint8)
        offsets = np.ascontiguousarray(offsets, dtype=np.int64)
        n = len(offsets) - 1
        words = np.zeros(len(data) // 64 + 1, np.uint64)
        self.lib.check(self.lib.L.tkz_pretokenize_utf8(self._h, _ptr(data), _ptr(offsets), n, _ptr(words)))
        bits = np.unpackbits(words.view(np.uint8), bitorder="little")
        return bits[:len(data) + 1].astype(bool)

    def encode_utf8(self, text: bytes):
        ids = np.empty(max(1, len(text)), np.int32)
        n = C.c_int64(0)
        buf = np.frombuffer(text, np.uint8) if text else np.zeros(1, np.uint8)
        self.lib.check(self.lib.L.tkz_encode_utf8(self._h, _ptr(buf), len(text), _ptr(ids), len(text), C.byref(n)))
        return ids[:n.value].tolist()

    def encode_utf16(self, units):
        u = np.ascontiguousarray(np.asarray(list(units) + [0], dtype=np.uint16))
        n_units = len(u) - 1
        ids = np.empty(max(1, 3 * n_units), np.int32)
        n = C.c_int64(0)
        self.lib.check(self.lib.L.tkz_encode_utf16(self._h, _ptr(u), n_units, _ptr(ids), 3 * n_units, C.byref(n)))
        return ids[:n.value].tolist()

    def encode_special(self, text: bytes, allowed, out_cap=None):
        """ITokenizer.Encode(text, allowedSpecial) on one string: tkz_encode_special_utf8.  allowed: indices as in encode_batch_special.  A TkzError of this
        call carries the count the entry reported as `needed` (E_CAPACITY: the required one)."""
        allowed = np.ascontiguousarray(allowed, dtype=np.int32)
        cap = len(text) if out_cap is None else out_cap
        ids = np.empty(max(1, cap), np.int32)
        n = C.c_int64(0)
        buf = np.frombuffer(text, np.uint8) if text else np.zeros(1, np.uint8)
        try:
            self.lib.check(self.lib.L.tkz_encode_special_utf8(self._h, _ptr(buf), len(text), _ptr(allowed) if len(allowed) else None, len(allowed), _ptr(ids), cap, C.byref(n)))
        except TkzError as ex:
            ex.needed = n.value
            raise
        return ids[:n.value].tolist()

    def encode_special_utf16(self, units, allowed, out_cap=None):
        """The same for a .NET `string` given as its UTF-16 code units: tkz_encode_special_utf16."""
        allowed = np.ascontiguousarray(allowed, dtype=np.int32)
        u = np.ascontiguousarray(np.asarray(list(units) + [0], dtype=np.uint16))
        n_units = len(u) - 1
        cap = 3 * n_units if out_cap is None else out_cap
        ids = np.empty(max(1, cap), np.int32)
        n = C.c_int64(0)
        try:
            self.lib.check(self.lib.L.tkz_encode_special_utf16(self._h, _ptr(u), n_units, _ptr(allowed) if len(allowed) else None, len(allowed), _ptr(ids), cap, C.byref(n)))
        except TkzError as ex:
            ex.needed = n.value
            raise
        return ids[:n.value].tolist()

    def encode_trim(self, text: bytes, allowed, side, max_tokens, out_cap=None):
        """EncodeTrimSuffix (side TRIM_SUFFIX) / EncodeTrimPrefix (TRIM_PREFIX) on one string: tkz_encode_trim_utf8.  (kept ids, cut_bytes, cut_units): the byte
        and UTF-16 length of the kept (suffix) or dropped (prefix) text.  allowed: indices as in encode_batch_special; out_cap counts the kept ids.  A TkzError
        of this call carries the count the entry reported as `needed` (E_CAPACITY: the kept one)."""
        allowed = np.ascontiguousarray(allowed, dtype=np.int32)
        cap = min(len(text), max(int(max_tokens), 0)) if out_cap is None else out_cap
        ids = np.empty(max(1, cap), np.int32)
        n, cb, cu = C.c_int64(0), C.c_int64(0), C.c_int64(0)
        buf = np.frombuffer(text, np.uint8) if text else np.zeros(1, np.uint8)
        try:
            self.lib.check(self.lib.L.tkz_encode_trim_utf8(self._h, _ptr(buf), len(text), _ptr(allowed) if len(allowed) else None, len(allowed), int(side), int(max_tokens),
                                                           _ptr(ids), cap, C.byref(n), C.byref(cb), C.byref(cu)))
        except TkzError as ex:
            ex.needed = n.value
            raise
        return ids[:n.value].tolist(), cb.value, cu.value

    def encode_trim_utf16(self, units, allowed, side, max_tokens, out_cap=None):
        """The same for a .NET `string` given as its UTF-16 code units: tkz_encode_trim_utf16.  (kept ids, cut_units)."""
        allowed = np.ascontiguousarray(allowed, dtype=np.int32)
        u = np.ascontiguousarray(np.asarray(list(units) + [0], dtype=np.uint16))
        n_units = len(u) - 1
        cap = min(3 * n_units, max(int(max_tokens), 0)) if out_cap is None else out_cap
        ids = np.empty(max(1, cap), np.int32)
        n, cu = C.c_int64(0), C.c_int64(0)
        try:
            self.lib.check(self.lib.L.tkz_encode_trim_utf16(self._h, _ptr(u), n_units, _ptr(allowed) if len(allowed) else None, len(allowed), int(side), int(max_tokens),
                                                            _ptr(ids), cap, C.byref(n), C.byref(cu)))
        except TkzError as ex:
            ex.needed = n.value
            raise
        return ids[:n.value].tolist(), cu.value

    # -- Decode --
    # -- counts: Encode(...).Count without the ids --
    def count_batch(self, data: np.ndarray, offsets: np.ndarray, allowed=()):
        """Token offsets int64[n+1] of the batch -- exactly encode_batch's / encode_batch_special's -- and no ids: tkz_count_batch_utf8.  The count of document d
        is offsets[d + 1] - offsets[d] (np.diff).  allowed: indices as in encode_batch_special."""
        data = np.ascontiguousarray(data, dtype=np.uint8)
        offsets = np.ascontiguousarray(offsets, dtype=np.int64)
        allowed = np.ascontiguousarray(allowed, dtype=np.int32)
        n = len(offsets) - 1
        ooff = np.empty(n + 1, np.int64)
        tot = C.c_int64(0)
        self.lib.check(self.lib.L.tkz_count_batch_utf8(self._h, _ptr(data) if len(data) else None, _ptr(offsets), n, _ptr(allowed) if len(allowed) else None, len(allowed),
                                                       _ptr(ooff), C.byref(tot)))
        return ooff

    def count_batch_utf16(self, units: np.ndarray, offsets: np.ndarray, allowed=()):
        """count_batch for UTF-16 documents (uint16[total], offsets in units): tkz_count_batch_utf16."""
        units = np.ascontiguousarray(units, dtype=np.uint16)
        offsets = np.ascontiguousarray(offsets, dtype=np.int64)
        allowed = np.ascontiguousarray(allowed, dtype=np.int32)
        n = len(offsets) - 1
        ooff = np.empty(n + 1, np.int64)
        tot = C.c_int64(0)
        buf = units if len(units) else np.zeros(1, np.uint16)
        self.lib.check(self.lib.L.tkz_count_batch_utf16(self._h, _ptr(buf), _ptr(offsets), n, _ptr(allowed) if len(allowed) else None, len(allowed), _ptr(ooff), C.byref(tot)))
        return ooff

    def count_batch_device(self, d_bytes, d_offsets, n_docs, total_bytes, allowed, d_out_offsets, stream=0):
        """Device buffers in, the token offsets (int64[n_docs + 1]) out, no id buffer: tkz_count_batch_device.  Returns the token total."""
        allowed = np.ascontiguousarray(allowed, dtype=np.int32)
        tot = C.c_int64(0)
        self.lib.check(self.lib.L.tkz_count_batch_device(self._h, d_bytes or None, d_offsets or None, n_docs, total_bytes, _ptr(allowed) if len(allowed) else None, len(allowed),
                                                         d_out_offsets or None, stream or None, C.byref(tot)))
        return tot.value

    def count(self, text: bytes, allowed=()):
        """len(encode_special(text, allowed)) without the ids: tkz_count_utf8."""
        allowed = np.ascontiguousarray(allowed, dtype=np.int32)
        n = C.c_int64(0)
        buf = np.frombuffer(text, np.uint8) if text else np.zeros(1, np.uint8)
        self.lib.check(self.lib.L.tkz_count_utf8(self._h, _ptr(buf), len(text), _ptr(allowed) if len(allowed) else None, len(allowed), C.byref(n)))
        return n.value

    def count_utf16(self, units, allowed=()):
        """The same for a .NET `string` given as its UTF-16 code units: tkz_count_utf16."""
        allowed = np.ascontiguousarray(allowed, dtype=np.int32)
        u = np.ascontiguousarray(np.asarray(list(units) + [0], dtype=np.uint16))
        n = C.c_int64(0)
        self.lib.check(self.lib.L.tkz_count_utf16(self._h, _ptr(u), len(u) - 1, _ptr(allowed) if len(allowed) else None, len(allowed), C.byref(n)))
        return n.value

    def count_calls(self):
        """(successful count calls, those of them the single-launch kernel answered)"""
        a, b = C.c_int64(0), C.c_int64(0)
        self.lib.L.tkz_encoder_count_calls(self._h, C.byref(a), C.byref(b))
        return a.value, b.value

    # -- token spans: the ids, and where every token's text starts in its document --
    def encode_batch_spans(self, data: np.ndarray, offsets: np.ndarray, allowed=(), want_bytes=True, want_units=True, out_cap=None):
        """(ids int32, offsets int64[n+1], tok_bytes int32 or None, tok_units int32 or None): the ids and offsets of encode_batch / encode_batch_special and, per
        token, the document-relative position of its first byte and the same position in UTF-16 code units: tkz_encode_batch_spans_utf8."""
        data = np.ascontiguousarray(data, dtype=np.uint8)
        offsets = np.ascontiguousarray(offsets, dtype=np.int64)
        allowed = np.ascontiguousarray(allowed, dtype=np.int32)
        n = len(offsets) - 1
        cap = len(data) if out_cap is None else out_cap
        ids = np.empty(max(1, cap), np.int32)
        tb = np.empty(max(1, cap), np.int32) if want_bytes else None
        tu = np.empty(max(1, cap), np.int32) if want_units else None
        ooff = np.empty(n + 1, np.int64)
        needed = C.c_int64(0)
        try:
            self.lib.check(self.lib.L.tkz_encode_batch_spans_utf8(self._h, _ptr(data) if len(data) else None, _ptr(offsets), n, _ptr(allowed) if len(allowed) else None,
                                                                  len(allowed), _ptr(ids), cap, _ptr(ooff), _ptr(tb) if want_bytes else None,
                                                                  _ptr(tu) if want_units else None, C.byref(needed)))
        except TkzError as ex:
            ex.needed = needed.value                          # (E_CAPACITY: the required count)
            raise
        k = needed.value
        return ids[:k], ooff, tb[:k] if want_bytes else None, tu[:k] if want_units else None

    def encode_batch_spans_utf16(self, units: np.ndarray, offsets: np.ndarray, allowed=(), out_cap=None):
        """encode_batch_spans for UTF-16 documents (uint16[total], offsets in units): (ids, offsets, tok_units) -- tkz_encode_batch_spans_utf16."""
        units = np.ascontiguousarray(units, dtype=np.uint16)
        offsets = np.ascontiguousarray(offsets, dtype=np.int64)
        allowed = np.ascontiguousarray(allowed, dtype=np.int32)
        n = len(offsets) - 1
        cap = 3 * len(units) if out_cap is None else out_cap
        ids = np.empty(max(1, cap), np.int32)
        tu = np.empty(max(1, cap), np.int32)
        ooff = np.empty(n + 1, np.int64)
        needed = C.c_int64(0)
        buf = units if len(units) else np.zeros(1, np.uint16)
        try:
            self.lib.check(self.lib.L.tkz_encode_batch_spans_utf16(self._h, _ptr(buf), _ptr(offsets), n, _ptr(allowed) if len(allowed) else None, len(allowed),
                                                                   _ptr(ids), cap, _ptr(ooff), _ptr(tu), C.byref(needed)))
        except TkzError as ex:
            ex.needed = needed.value
            raise
        return ids[:needed.value], ooff, tu[:needed.value]

    def encode_batch_spans_device(self, d_bytes, d_offsets, n_docs, total_bytes, allowed, d_out_ids, out_cap, d_out_offsets, d_tok_bytes=0, d_tok_units=0, stream=0):
        """Device buffers in and out: tkz_encode_batch_spans_device.  Returns the token total; a TkzError carries it as `needed`."""
        allowed = np.ascontiguousarray(allowed, dtype=np.int32)
        tot = C.c_int64(0)
        try:
            self.lib.check(self.lib.L.tkz_encode_batch_spans_device(self._h, d_bytes or None, d_offsets or None, n_docs, total_bytes, _ptr(allowed) if len(allowed) else None,
                                                                    len(allowed), d_out_ids or None, out_cap, d_out_offsets or None, d_tok_bytes or None,
                                                                    d_tok_units or None, stream or None, C.byref(tot)))
        except TkzError as ex:
            ex.needed = tot.value
            raise
        return tot.value

    def encode_spans(self, text: bytes, allowed=(), want_bytes=True, want_units=True, out_cap=None):
        """ONE text: (ids, tok_bytes or None, tok_units or None) as lists -- tkz_encode_spans_utf8."""
        allowed = np.ascontiguousarray(allowed, dtype=np.int32)
        cap = len(text) if out_cap is None else out_cap
        ids = np.empty(max(1, cap), np.int32)
        tb = np.empty(max(1, cap), np.int32) if want_bytes else None
        tu = np.empty(max(1, cap), np.int32) if want_units else None
        n = C.c_int64(0)
        buf = np.frombuffer(text, np.uint8) if text else np.zeros(1, np.uint8)
        try:
            self.lib.check(self.lib.L.tkz_encode_spans_utf8(self._h, _ptr(buf), len(text), _ptr(allowed) if len(allowed) else None, len(allowed), _ptr(ids), cap,
                                                            _ptr(tb) if want_bytes else None, _ptr(tu) if want_units else None, C.byref(n)))
        except TkzError as ex:
            ex.needed = n.value
            raise
        k = n.value
        return ids[:k].tolist(), tb[:k].tolist() if want_bytes else None, tu[:k].tolist() if want_units else None

    def encode_spans_utf16(self, units, allowed=(), out_cap=None):
        """The same for a .NET `string` given as its UTF-16 code units: (ids, tok_units) -- tkz_encode_spans_utf16."""
        allowed = np.ascontiguousarray(allowed, dtype=np.int32)
        u = np.ascontiguousarray(np.asarray(list(units) + [0], dtype=np.uint16))
        n_units = len(u) - 1
        cap = 3 * n_units if out_cap is None else out_cap
        ids = np.empty(max(1, cap), np.int32)
        tu = np.empty(max(1, cap), np.int32)
        n = C.c_int64(0)
        try:
            self.lib.check(self.lib.L.tkz_encode_spans_utf16(self._h, _ptr(u), n_units, _ptr(allowed) if len(allowed) else None, len(allowed), _ptr(ids), cap, _ptr(tu),
                                                             C.byref(n)))
        except TkzError as ex:
            ex.needed = n.value
            raise
        return ids[:n.value].tolist(), tu[:n.value].tolist()

    def spans_calls(self):
        """successful calls of the span entries"""
        a = C.c_int64(0)
        self.lib.L.tkz_encoder_spans_calls(self._h, C.byref(a))
        return a.value

    # -- token-budget chunks: the ids, and every document's tokens cut into chunks of at most max_tokens (tkz.h: the rule) --
    @staticmethod
    def chunk_bound(n_docs, total, max_tokens):
        """chunks that always suffice (tkz.h), and never more than a chunk a byte"""
        return max(0, min(total, n_docs + 2 * total // max(1, max_tokens)))

    def _chunks_call(self, fn, head, max_tokens, n, cap, ccap, want_bytes, want_units, batch):
        """the shared tail of the host entries: (ids, offsets or None, doc_chunk_offsets or None, chunk_tokens, chunk_bytes or None, chunk_units or None)"""
        ids = np.empty(max(1, cap), np.int32)
        ct = np.empty(max(1, ccap) + 1, np.int64)
        cb = np.empty(max(1, ccap), np.int64) if want_bytes else None
        cu = np.empty(max(1, ccap), np.int64) if want_units else None
        ooff, dco = (np.empty(n + 1, np.int64), np.empty(n + 1, np.int64)) if batch else (None, None)
        ni, nc = C.c_int64(0), C.c_int64(0)
        args = list(head) + [max_tokens, _ptr(ids), cap]
        if batch:
            args += [_ptr(ooff), _ptr(dco)]
        args += [_ptr(ct)] + ([_ptr(cb) if want_bytes else None] if want_bytes is not None else []) + [_ptr(cu) if want_units else None, ccap, C.byref(ni), C.byref(nc)]
        try:
            self.lib.check(fn(self._h, *args))
        except TkzError as ex:
            ex.needed, ex.needed_chunks = ni.value, nc.value          # (E_CAPACITY: the required counts)
            raise
        k, c = ni.value, nc.value
        return ids[:k], ooff, dco, ct[:c + 1], cb[:c] if want_bytes else None, cu[:c] if want_units else None

    def encode_batch_chunks(self, data: np.ndarray, offsets: np.ndarray, max_tokens, allowed=(), want_bytes=True, want_units=True, out_cap=None, chunk_cap=None):
        """(ids int32, offsets int64[n+1], doc_chunk_offsets int64[n+1], chunk_tokens int64[chunks+1], chunk_bytes int64 or None, chunk_units int64 or None): the ids
        and offsets of encode_batch / encode_batch_special and the chunk table -- tkz_encode_batch_chunks_utf8."""
        data = np.ascontiguousarray(data, dtype=np.uint8)
        offsets = np.ascontiguousarray(offsets, dtype=np.int64)
        allowed = np.ascontiguousarray(allowed, dtype=np.int32)
        n = len(offsets) - 1
        cap = len(data) if out_cap is None else out_cap
        ccap = self.chunk_bound(n, len(data), max_tokens) if chunk_cap is None else chunk_cap
        head = [_ptr(data) if len(data) else None, _ptr(offsets), n, _ptr(allowed) if len(allowed) else None, len(allowed)]
        return self._chunks_call(self.lib.L.tkz_encode_batch_chunks_utf8, head, max_tokens, n, cap, ccap, bool(want_bytes), want_units, True)

    def encode_batch_chunks_utf16(self, units: np.ndarray, offsets: np.ndarray, max_tokens, allowed=(), out_cap=None, chunk_cap=None):
        """encode_batch_chunks for UTF-16 documents (uint16[total], offsets in units): (ids, offsets, doc_chunk_offsets, chunk_tokens, chunk_units) --
        tkz_encode_batch_chunks_utf16."""
        units = np.ascontiguousarray(units, dtype=np.uint16)
        offsets = np.ascontiguousarray(offsets, dtype=np.int64)
        allowed = np.ascontiguousarray(allowed, dtype=np.int32)
        n = len(offsets) - 1
        cap = 3 * len(units) if out_cap is None else out_cap
        ccap = self.chunk_bound(n, 3 * len(units), max_tokens) if chunk_cap is None else chunk_cap
        buf = units if len(units) else np.zeros(1, np.uint16)
        head = [_ptr(buf), _ptr(offsets), n, _ptr(allowed) if len(allowed) else None, len(allowed)]
        r = self._chunks_call(self.lib.L.tkz_encode_batch_chunks_utf16, head, max_tokens, n, cap, ccap, None, True, True)
        return r[0], r[1], r[2], r[3], r[5]

    def encode_batch_chunks_device(self, d_bytes, d_offsets, n_docs, total_bytes, max_tokens, allowed, d_out_ids, out_cap, d_out_offsets, d_doc_chunk_offsets,
                                   d_chunk_tokens, d_chunk_bytes=0, d_chunk_units=0, chunk_cap=0, stream=0):
        """Device buffers in and out: tkz_encode_batch_chunks_device.  Returns (token total, chunks); a TkzError carries them as `needed` and `needed_chunks`."""
        allowed = np.ascontiguousarray(allowed, dtype=np.int32)
        tot, nch = C.c_int64(0), C.c_int64(0)
        try:
            self.lib.check(self.lib.L.tkz_encode_batch_chunks_device(self._h, d_bytes or None, d_offsets or None, n_docs, total_bytes, _ptr(allowed) if len(allowed) else None,
                                                                     len(allowed), max_tokens, d_out_ids or None, out_cap, d_out_offsets or None, d_doc_chunk_offsets or None,
                                                                     d_chunk_tokens or None, d_chunk_bytes or None, d_chunk_units or None, chunk_cap, stream or None,
                                                                     C.byref(tot), C.byref(nch)))
        except TkzError as ex:
            ex.needed, ex.needed_chunks = tot.value, nch.value
            raise
        return tot.value, nch.value

    def encode_chunks(self, text: bytes, max_tokens, allowed=(), want_bytes=True, want_units=True, out_cap=None, chunk_cap=None):
        """ONE text: (ids, chunk_tokens, chunk_bytes or None, chunk_units or None) as lists -- tkz_encode_chunks_utf8."""
        allowed = np.ascontiguousarray(allowed, dtype=np.int32)
        cap = len(text) if out_cap is None else out_cap
        ccap = self.chunk_bound(1, len(text), max_tokens) if chunk_cap is None else chunk_cap
        buf = np.frombuffer(text, np.uint8) if text else np.zeros(1, np.uint8)
        head = [_ptr(buf), len(text), _ptr(allowed) if len(allowed) else None, len(allowed)]
        r = self._chunks_call(self.lib.L.tkz_encode_chunks_utf8, head, max_tokens, 1, cap, ccap, bool(want_bytes), want_units, False)
        return r[0].tolist(), r[3].tolist(), r[4].tolist() if want_bytes else None, r[5].tolist() if want_units else None

    def encode_chunks_utf16(self, units, max_tokens, allowed=(), out_cap=None, chunk_cap=None):
        """The same for a .NET `string` given as its UTF-16 code units: (ids, chunk_tokens, chunk_units) -- tkz_encode_chunks_utf16."""
        allowed = np.ascontiguousarray(allowed, dtype=np.int32)
        u = np.ascontiguousarray(np.asarray(list(units) + [0], dtype=np.uint16))
        n_units = len(u) - 1
        cap = 3 * n_units if out_cap is None else out_cap
        ccap = self.chunk_bound(1, 3 * n_units, max_tokens) if chunk_cap is None else chunk_cap
        head = [_ptr(u), n_units, _ptr(allowed) if len(allowed) else None, len(allowed)]
        r = self._chunks_call(self.lib.L.tkz_encode_chunks_utf16, head, max_tokens, 1, cap, ccap, None, True, False)
        return r[0].tolist(), r[3].tolist(), r[5].tolist()

    def chunks_calls(self):
        """successful calls of the chunk entries"""
        a = C.c_int64(0)
        self.lib.L.tkz_encoder_chunks_calls(self._h, C.byref(a))
        return a.value

    # -- overlapping token-budget chunks: a chunk size and an overlap; every chunk has a start and an end in the table (tkz.h: the rule) --
    @staticmethod
    def chunk_bound_overlap(n_docs, total, max_tokens, overlap):
        """chunks that always suffice (tkz.h: chunk_bound with max_tokens - overlap in the place of max_tokens), and never more than a chunk a byte"""
        return max(0, min(total, n_docs + 2 * total // max(1, max_tokens - overlap)))

    def _chunks_overlap_call(self, fn, head, max_tokens, overlap, n, cap, ccap, want, batch):
        """the shared tail of the host entries.  want: (bytes, units, end_bytes, end_units), None for an array the entry does not have.  Returns (ids, offsets or
        None, doc_chunk_offsets or None, chunk_tokens, chunk_ends, [chunk_bytes, chunk_units, chunk_end_bytes, chunk_end_units] with None where not asked for)"""
        ids = np.empty(max(1, cap), np.int32)
        ct, ce = np.empty(max(1, ccap), np.int64), np.empty(max(1, ccap), np.int64)
        pos = [np.empty(max(1, ccap), np.int64) if w else None for w in want]
        ooff, dco = (np.empty(n + 1, np.int64), np.empty(n + 1, np.int64)) if batch else (None, None)
        ni, nc = C.c_int64(0), C.c_int64(0)
        args = list(head) + [max_tokens, overlap, _ptr(ids), cap]
        if batch:
            args += [_ptr(ooff), _ptr(dco)]
        args += [_ptr(ct), _ptr(ce)] + [_ptr(a) if a is not None else None for a, w in zip(pos, want) if w is not None] + [ccap, C.byref(ni), C.byref(nc)]
        try:
            self.lib.check(fn(self._h, *args))
        except TkzError as ex:
            ex.needed, ex.needed_chunks = ni.value, nc.value          # (E_CAPACITY: the required counts)
            raise
        k, c = ni.value, nc.value
        return ids[:k], ooff, dco, ct[:c], ce[:c], [a[:c] if a is not None else None for a in pos]

    def encode_batch_chunks_overlap(self, data: np.ndarray, offsets: np.ndarray, max_tokens, overlap, allowed=(), want=(True, True, True, True), out_cap=None,
                                    chunk_cap=None):
        """(ids int32, offsets int64[n+1], doc_chunk_offsets int64[n+1], chunk_tokens int64[chunks], chunk_ends int64[chunks], chunk_bytes, chunk_units,
        chunk_end_bytes, chunk_end_units -- int64[chunks] or None, by `want`) -- tkz_encode_batch_chunks_overlap_utf8."""
        data = np.ascontiguousarray(data, dtype=np.uint8)
        offsets = np.ascontiguousarray(offsets, dtype=np.int64)
        allowed = np.ascontiguousarray(allowed, dtype=np.int32)
        n = len(offsets) - 1
        cap = len(data) if out_cap is None else out_cap
        ccap = self.chunk_bound_overlap(n, len(data), max_tokens, overlap) if chunk_cap is None else chunk_cap
        head = [_ptr(data) if len(data) else None, _ptr(offsets), n, _ptr(allowed) if len(allowed) else None, len(allowed)]
        r = self._chunks_overlap_call(self.lib.L.tkz_encode_batch_chunks_overlap_utf8, head, max_tokens, overlap, n, cap, ccap, [bool(w) for w in want], True)
        return (r[0], r[1], r[2], r[3], r[4]) + tuple(r[5])

    def encode_batch_chunks_overlap_utf16(self, units: np.ndarray, offsets: np.ndarray, max_tokens, overlap, allowed=(), want=(True, True), out_cap=None, chunk_cap=None):
        """The same for UTF-16 documents (uint16[total], offsets in units): (ids, offsets, doc_chunk_offsets, chunk_tokens, chunk_ends, chunk_units, chunk_end_units)
        -- tkz_encode_batch_chunks_overlap_utf16."""
        units = np.ascontiguousarray(units, dtype=np.uint16)
        offsets = np.ascontiguousarray(offsets, dtype=np.int64)
        allowed = np.ascontiguousarray(allowed, dtype=np.int32)
        n = len(offsets) - 1
        cap = 3 * len(units) if out_cap is None else out_cap
        ccap = self.chunk_bound_overlap(n, 3 * len(units), max_tokens, overlap) if chunk_cap is None else chunk_cap
        buf = units if len(units) else np.zeros(1, np.uint16)
        head = [_ptr(buf), _ptr(offsets), n, _ptr(allowed) if len(allowed) else None, len(allowed)]
        r = self._chunks_overlap_call(self.lib.L.tkz_encode_batch_chunks_overlap_utf16, head, max_tokens, overlap, n, cap, ccap,
                                      [None, bool(want[0]), None, bool(want[1])], True)
        return r[0], r[1], r[2], r[3], r[4], r[5][1], r[5][3]

    def encode_batch_chunks_overlap_device(self, d_bytes, d_offsets, n_docs, total_bytes, max_tokens, overlap, allowed, d_out_ids, out_cap, d_out_offsets,
                                           d_doc_chunk_offsets, d_chunk_tokens, d_chunk_ends, d_chunk_bytes=0, d_chunk_units=0, d_chunk_end_bytes=0, d_chunk_end_units=0,
                                           chunk_cap=0, stream=0):
        """Device buffers in and out: tkz_encode_batch_chunks_overlap_device.  Returns (token total, chunks); a TkzError carries them as `needed` and `needed_chunks`."""
        allowed = np.ascontiguousarray(allowed, dtype=np.int32)
        tot, nch = C.c_int64(0), C.c_int64(0)
        try:
            self.lib.check(self.lib.L.tkz_encode_batch_chunks_overlap_device(
                self._h, d_bytes or None, d_offsets or None, n_docs, total_bytes, _ptr(allowed) if len(allowed) else None, len(allowed), max_tokens, overlap,
                d_out_ids or None, out_cap, d_out_offsets or None, d_doc_chunk_offsets or None, d_chunk_tokens or None, d_chunk_ends or None, d_chunk_bytes or None,
                d_chunk_units or None, d_chunk_end_bytes or None, d_chunk_end_units or None, chunk_cap, stream or None, C.byref(tot), C.byref(nch)))
        except TkzError as ex:
            ex.needed, ex.needed_chunks = tot.value, nch.value
            raise
        return tot.value, nch.value

    def encode_chunks_overlap(self, text: bytes, max_tokens, overlap, allowed=(), want=(True, True, True, True), out_cap=None, chunk_cap=None):
        """ONE text: (ids, chunk_tokens, chunk_ends, chunk_bytes, chunk_units, chunk_end_bytes, chunk_end_units) as lists (None where not asked for) --
        tkz_encode_chunks_overlap_utf8."""
        allowed = np.ascontiguousarray(allowed, dtype=np.int32)
        cap = len(text) if out_cap is None else out_cap
        ccap = self.chunk_bound_overlap(1, len(text), max_tokens, overlap) if chunk_cap is None else chunk_cap
        buf = np.frombuffer(text, np.uint8) if text else np.zeros(1, np.uint8)
        head = [_ptr(buf), len(text), _ptr(allowed) if len(allowed) else None, len(allowed)]
        r = self._chunks_overlap_call(self.lib.L.tkz_encode_chunks_overlap_utf8, head, max_tokens, overlap, 1, cap, ccap, [bool(w) for w in want], False)
        return (r[0].tolist(), r[3].tolist(), r[4].tolist()) + tuple(a.tolist() if a is not None else None for a in r[5])

    def encode_chunks_overlap_utf16(self, units, max_tokens, overlap, allowed=(), out_cap=None, chunk_cap=None):
        """The same for a .NET `string` given as its UTF-16 code units: (ids, chunk_tokens, chunk_ends, chunk_units, chunk_end_units) --
        tkz_encode_chunks_overlap_utf16."""
        allowed = np.ascontiguousarray(allowed, dtype=np.int32)
        u = np.ascontiguousarray(np.asarray(list(units) + [0], dtype=np.uint16))
        n_units = len(u) - 1
        cap = 3 * n_units if out_cap is None else out_cap
        ccap = self.chunk_bound_overlap(1, 3 * n_units, max_tokens, overlap) if chunk_cap is None else chunk_cap
        head = [_ptr(u), n_units, _ptr(allowed) if len(allowed) else None, len(allowed)]
        r = self._chunks_overlap_call(self.lib.L.tkz_encode_chunks_overlap_utf16, head, max_tokens, overlap, 1, cap, ccap, [None, True, None, True], False)
        return r[0].tolist(), r[3].tolist(), r[4].tolist(), r[5][1].tolist(), r[5][3].tolist()

    def chunks_overlap_calls(self):
        """successful calls of the overlap chunk entries"""
        a = C.c_int64(0)
        self.lib.L.tkz_encoder_chunks_overlap_calls(self._h, C.byref(a))
        return a.value

    # -- packed rows: the ids framed by bos / eos ids and laid out in rows of row_len, with pos and seg_starts (tkz.h: the rule) --
    @staticmethod
    def packed_bounds(n_docs, total, row_len, framing):
        """(ids, segments) that always suffice (tkz.h): the stream bound rounded up to whole rows, and a segment a document and a row"""
        rows = -(-(total + framing * n_docs) // row_len)
        return rows * row_len, n_docs + rows

    def _packed_host(self, fn, buf, offsets, total, allowed, row_len, bos_id, eos_id, pad_id, want_pos, want_segs, out_cap, seg_cap):
        offsets = np.ascontiguousarray(offsets, dtype=np.int64)
        allowed = np.ascontiguousarray(allowed, dtype=np.int32)
        n = len(offsets) - 1
        if row_len >= 1:
            bound, sbound = self.packed_bounds(n, total, row_len, (bos_id >= 0) + (eos_id >= 0))
        else:
            bound = sbound = 0                                # (refused by the library)
        cap = bound if out_cap is None else out_cap
        scap = sbound if seg_cap is None else seg_cap
        ids = np.empty(max(1, cap), np.int32)
        pos = np.empty(max(1, cap), np.int32) if want_pos else None
        seg = np.empty(max(0, scap) + 1, np.int64) if want_segs else None
        ooff = np.empty(n + 1, np.int64)
        tot, ni, ns = C.c_int64(0), C.c_int64(0), C.c_int64(0)
        try:
            self.lib.check(fn(self._h, buf, _ptr(offsets), n, _ptr(allowed) if len(allowed) else None, len(allowed), bos_id, eos_id, row_len, pad_id, _ptr(ids), cap,
                              _ptr(ooff), _ptr(pos) if want_pos else None, _ptr(seg) if want_segs else None, scap, C.byref(tot), C.byref(ni), C.byref(ns)))
        except TkzError as ex:
            ex.needed, ex.needed_ids, ex.needed_segs = tot.value, ni.value, ns.value      # (E_CAPACITY: the required figures)
            raise
        k, rows = ni.value, ni.value // row_len
        return (ids[:k].reshape(rows, row_len), ooff, pos[:k].reshape(rows, row_len) if want_pos else None, seg[:ns.value + 1] if want_segs else None, tot.value)

    def encode_batch_packed(self, data: np.ndarray, offsets: np.ndarray, row_len, allowed=(), bos_id=-1, eos_id=-1, pad_id=0, want_pos=True, want_segs=True,
                            out_cap=None, seg_cap=None):
        """(ids int32[n_rows, row_len], offsets int64[n+1], pos int32[n_rows, row_len] or None, seg_starts int64[n_segs + 1] or None, T): the ids of encode_batch /
        encode_batch_special framed and laid out in rows -- tkz_encode_batch_packed_utf8."""
        data = np.ascontiguousarray(data, dtype=np.uint8)
        return self._packed_host(self.lib.L.tkz_encode_batch_packed_utf8, _ptr(data) if len(data) else None, offsets, len(data), allowed, row_len, bos_id, eos_id, pad_id,
                                 want_pos, want_segs, out_cap, seg_cap)

    def encode_batch_packed_utf16(self, units: np.ndarray, offsets: np.ndarray, row_len, allowed=(), bos_id=-1, eos_id=-1, pad_id=0, want_pos=True, want_segs=True,
                                  out_cap=None, seg_cap=None):
        """encode_batch_packed for UTF-16 documents (uint16[total], offsets in units) -- tkz_encode_batch_packed_utf16."""
        units = np.ascontiguousarray(units, dtype=np.uint16)
        buf = units if len(units) else np.zeros(1, np.uint16)
        return self._packed_host(self.lib.L.tkz_encode_batch_packed_utf16, _ptr(buf), offsets, 3 * len(units), allowed, row_len, bos_id, eos_id, pad_id,
                                 want_pos, want_segs, out_cap, seg_cap)

    def encode_batch_packed_device(self, d_bytes, d_offsets, n_docs, total_bytes, allowed, bos_id, eos_id, row_len, pad_id, d_out_ids, out_cap, d_out_offsets,
                                   d_pos=0, d_seg_starts=0, seg_cap=0, stream=0):
        """Device buffers in and out: tkz_encode_batch_packed_device.  Returns (T, n_rows, n_segs); a TkzError carries them as `needed`, `needed_rows`, `needed_segs`."""
        allowed = np.ascontiguousarray(allowed, dtype=np.int32)
        tot, rows, segs = C.c_int64(0), C.c_int64(0), C.c_int64(0)
        try:
            self.lib.check(self.lib.L.tkz_encode_batch_packed_device(self._h, d_bytes or None, d_offsets or None, n_docs, total_bytes, _ptr(allowed) if len(allowed) else None,
                                                                     len(allowed), bos_id, eos_id, row_len, pad_id, d_out_ids or None, out_cap, d_out_offsets or None,
                                                                     d_pos or None, d_seg_starts or None, seg_cap, stream or None, C.byref(tot), C.byref(rows), C.byref(segs)))
        except TkzError as ex:
            ex.needed, ex.needed_rows, ex.needed_segs = tot.value, rows.value, segs.value
            raise
        return tot.value, rows.value, segs.value

    def packed_calls(self):
        """successful calls of the packed entries"""
        a = C.c_int64(0)
        self.lib.L.tkz_encoder_packed_calls(self._h, C.byref(a))
        return a.value

    # -- padded rows: a row a document, cut to max_len, framed by bos / eos ids, padded to the common width, with mask, pos and lens (tkz.h: the rule) --
    @staticmethod
    def padded_bounds(n_docs, max_len):
        """the ids (and mask bytes, and pos entries) that always suffice (tkz.h): a row of max_len a document"""
        return n_docs * max_len

    def _padded_host(self, fn, buf, offsets, allowed, max_len, bos_id, eos_id, pad_id, cut_side, pad_side, pad_multiple, want_mask, want_pos, want_offs, out_cap):
        offsets = np.ascontiguousarray(offsets, dtype=np.int64)
        allowed = np.ascontiguousarray(allowed, dtype=np.int32)
        n = len(offsets) - 1
        cap = (self.padded_bounds(n, max_len) if 1 <= max_len < 1 << 31 else 0) if out_cap is None else out_cap      # (a max_len out of range is refused by the library)
        ids = np.empty(max(1, cap), np.int32)
        mask = np.empty(max(1, cap), np.uint8) if want_mask else None
        pos = np.empty(max(1, cap), np.int32) if want_pos else None
        lens = np.empty(max(1, n), np.int32)
        ooff = np.empty(n + 1, np.int64) if want_offs else None
        tot, w, cut = C.c_int64(0), C.c_int64(0), C.c_int64(0)
        try:
            self.lib.check(fn(self._h, buf, _ptr(offsets), n, _ptr(allowed) if len(allowed) else None, len(allowed), bos_id, eos_id, max_len, cut_side, pad_side, pad_id,
                              pad_multiple, _ptr(ids), cap, _ptr(mask) if want_mask else None, _ptr(pos) if want_pos else None, _ptr(lens), _ptr(ooff) if want_offs else None,
                              C.byref(tot), C.byref(w), C.byref(cut)))
        except TkzError as ex:
            ex.needed, ex.needed_width, ex.n_cut = tot.value, w.value, cut.value      # (E_CAPACITY: the required figures)
            raise
        W = w.value
        return (ids[:n * W].reshape(n, W), mask[:n * W].reshape(n, W) if want_mask else None, pos[:n * W].reshape(n, W) if want_pos else None, lens[:n], ooff,
                tot.value, cut.value)

    def encode_batch_padded(self, data: np.ndarray, offsets: np.ndarray, max_len, allowed=(), bos_id=-1, eos_id=-1, pad_id=0, cut_side=TRIM_SUFFIX, pad_side=PAD_RIGHT,
                            pad_multiple=1, want_mask=True, want_pos=True, want_offs=True, out_cap=None):
        """(ids int32[n, W], mask uint8[n, W] or None, pos int32[n, W] or None, lens int32[n], offsets int64[n + 1] or None, total_tokens, n_cut): the ids of
        encode_batch / encode_batch_special cut to max_len, framed and padded to the common width W -- tkz_encode_batch_padded_utf8."""
        data = np.ascontiguousarray(data, dtype=np.uint8)
        return self._padded_host(self.lib.L.tkz_encode_batch_padded_utf8, _ptr(data) if len(data) else None, offsets, allowed, max_len, bos_id, eos_id, pad_id, cut_side,
                                 pad_side, pad_multiple, want_mask, want_pos, want_offs, out_cap)

    def encode_batch_padded_utf16(self, units: np.ndarray, offsets: np.ndarray, max_len, allowed=(), bos_id=-1, eos_id=-1, pad_id=0, cut_side=TRIM_SUFFIX, pad_side=PAD_RIGHT,
                                  pad_multiple=1, want_mask=True, want_pos=True, want_offs=True, out_cap=None):
        """encode_batch_padded for UTF-16 documents (uint16[total], offsets in units) -- tkz_encode_batch_padded_utf16."""
        units = np.ascontiguousarray(units, dtype=np.uint16)
        buf = units if len(units) else np.zeros(1, np.uint16)
        return self._padded_host(self.lib.L.tkz_encode_batch_padded_utf16, _ptr(buf), offsets, allowed, max_len, bos_id, eos_id, pad_id, cut_side, pad_side, pad_multiple,
                                 want_mask, want_pos, want_offs, out_cap)

    def encode_batch_padded_device(self, d_bytes, d_offsets, n_docs, total_bytes, allowed, bos_id, eos_id, max_len, cut_side, pad_side, pad_id, pad_multiple, d_out_ids, out_cap,
                                   d_mask=0, d_pos=0, d_lens=0, d_out_offsets=0, stream=0):
        """Device buffers in and out: tkz_encode_batch_padded_device.  Returns (total_tokens, W, n_cut); a TkzError carries them as `needed`, `needed_width`, `n_cut`."""
        allowed = np.ascontiguousarray(allowed, dtype=np.int32)
        tot, w, cut = C.c_int64(0), C.c_int64(0), C.c_int64(0)
        try:
            self.lib.check(self.lib.L.tkz_encode_batch_padded_device(self._h, d_bytes or None, d_offsets or None, n_docs, total_bytes, _ptr(allowed) if len(allowed) else None,
                                                                     len(allowed), bos_id, eos_id, max_len, cut_side, pad_side, pad_id, pad_multiple, d_out_ids or None, out_cap,
                                                                     d_mask or None, d_pos or None, d_lens or None, d_out_offsets or None, stream or None,
                                                                     C.byref(tot), C.byref(w), C.byref(cut)))
        except TkzError as ex:
            ex.needed, ex.needed_width, ex.n_cut = tot.value, w.value, cut.value
            raise
        return tot.value, w.value, cut.value

    def padded_calls(self):
        """successful calls of the padded entries"""
        a = C.c_int64(0)
        self.lib.L.tkz_encoder_padded_calls(self._h, C.byref(a))
        return a.value

    # -- length-bucketed padded rows: the padded rows of the documents sorted by len, every bucket of bucket_rows rows at its own width (tkz.h: the rule) --
    @staticmethod
    def bucket_count(n_docs, bucket_rows):
        """n_buckets = ceil(n_docs / bucket_rows) (tkz.h): the caller sizes the bucket arrays from it"""
        return -(-n_docs // bucket_rows) if bucket_rows >= 1 else 0

    def _bucketed_host(self, fn, buf, offsets, allowed, max_len, bucket_rows, order, bos_id, eos_id, pad_id, cut_side, pad_side, pad_multiple, want_mask, want_pos, want_offs,
                       want_rank, out_cap):
        offsets = np.ascontiguousarray(offsets, dtype=np.int64)
        allowed = np.ascontiguousarray(allowed, dtype=np.int32)
        n = len(offsets) - 1
        nb = self.bucket_count(n, bucket_rows)
        cap = (self.padded_bounds(n, max_len) if 1 <= max_len < 1 << 31 else 0) if out_cap is None else out_cap      # (a max_len out of range is refused by the library)
        ids = np.empty(max(1, cap), np.int32)
        mask = np.empty(max(1, cap), np.uint8) if want_mask else None
        pos = np.empty(max(1, cap), np.int32) if want_pos else None
        lens = np.empty(max(1, n), np.int32)
        ooff = np.empty(n + 1, np.int64) if want_offs else None
        perm = np.empty(max(1, n), np.int64)
        rank = np.empty(max(1, n), np.int64) if want_rank else None
        boffs = np.empty(nb + 1, np.int64)
        widths = np.empty(max(1, nb), np.int32)
        tot, p, cut = C.c_int64(0), C.c_int64(0), C.c_int64(0)
        try:
            self.lib.check(fn(self._h, buf, _ptr(offsets), n, _ptr(allowed) if len(allowed) else None, len(allowed), bos_id, eos_id, max_len, cut_side, pad_side, pad_id,
                              pad_multiple, bucket_rows, order, _ptr(ids), cap, _ptr(mask) if want_mask else None, _ptr(pos) if want_pos else None, _ptr(lens),
                              _ptr(ooff) if want_offs else None, _ptr(perm), _ptr(rank) if want_rank else None, _ptr(boffs), _ptr(widths), C.byref(tot), C.byref(p),
                              C.byref(cut)))
        except TkzError as ex:
            ex.needed, ex.needed_positions, ex.n_cut = tot.value, p.value, cut.value      # (E_CAPACITY: the required figures)
            raise
        P = p.value
        return (ids[:P], mask[:P] if want_mask else None, pos[:P] if want_pos else None, lens[:n], ooff, perm[:n], rank[:n] if want_rank else None, boffs, widths[:nb],
                tot.value, cut.value)

    def encode_batch_bucketed(self, data: np.ndarray, offsets: np.ndarray, max_len, bucket_rows, order=BUCKET_ASCENDING, allowed=(), bos_id=-1, eos_id=-1, pad_id=0,
                              cut_side=TRIM_SUFFIX, pad_side=PAD_RIGHT, pad_multiple=1, want_mask=True, want_pos=True, want_offs=True, want_rank=True, out_cap=None):
        """(ids int32[P], mask uint8[P] or None, pos int32[P] or None, lens int32[n], offsets int64[n + 1] or None, order int64[n], rank int64[n] or None,
        bucket_offsets int64[n_buckets + 1], bucket_widths int32[n_buckets], total_tokens, n_cut): the padded rows of the documents sorted by len, bucket b of
        bucket_rows rows at ids[bucket_offsets[b] : bucket_offsets[b + 1]] with its own width -- tkz_encode_batch_bucketed_utf8."""
        data = np.ascontiguousarray(data, dtype=np.uint8)
        return self._bucketed_host(self.lib.L.tkz_encode_batch_bucketed_utf8, _ptr(data) if len(data) else None, offsets, allowed, max_len, bucket_rows, order, bos_id, eos_id,
                                   pad_id, cut_side, pad_side, pad_multiple, want_mask, want_pos, want_offs, want_rank, out_cap)

    def encode_batch_bucketed_utf16(self, units: np.ndarray, offsets: np.ndarray, max_len, bucket_rows, order=BUCKET_ASCENDING, allowed=(), bos_id=-1, eos_id=-1, pad_id=0,
                                    cut_side=TRIM_SUFFIX, pad_side=PAD_RIGHT, pad_multiple=1, want_mask=True, want_pos=True, want_offs=True, want_rank=True, out_cap=None):
        """encode_batch_bucketed for UTF-16 documents (uint16[total], offsets in units) -- tkz_encode_batch_bucketed_utf16."""
        units = np.ascontiguousarray(units, dtype=np.uint16)
        buf = units if len(units) else np.zeros(1, np.uint16)
        return self._bucketed_host(self.lib.L.tkz_encode_batch_bucketed_utf16, _ptr(buf), offsets, allowed, max_len, bucket_rows, order, bos_id, eos_id, pad_id, cut_side,
                                   pad_side, pad_multiple, want_mask, want_pos, want_offs, want_rank, out_cap)

    def encode_batch_bucketed_device(self, d_bytes, d_offsets, n_docs, total_bytes, allowed, bos_id, eos_id, max_len, cut_side, pad_side, pad_id, pad_multiple, bucket_rows,
                                     order, d_out_ids, out_cap, d_mask=0, d_pos=0, d_lens=0, d_out_offsets=0, d_order=0, d_rank=0, d_bucket_offsets=0, d_bucket_widths=0,
                                     stream=0):
        """Device buffers in and out: tkz_encode_batch_bucketed_device.  Returns (total_tokens, P, n_cut); a TkzError carries them as `needed`,
        `needed_positions`, `n_cut`."""
        allowed = np.ascontiguousarray(allowed, dtype=np.int32)
        tot, p, cut = C.c_int64(0), C.c_int64(0), C.c_int64(0)
        try:
            self.lib.check(self.lib.L.tkz_encode_batch_bucketed_device(self._h, d_bytes or None, d_offsets or None, n_docs, total_bytes, _ptr(allowed) if len(allowed) else None,
                                                                       len(allowed), bos_id, eos_id, max_len, cut_side, pad_side, pad_id, pad_multiple, bucket_rows, order,
                                                                       d_out_ids or None, out_cap, d_mask or None, d_pos or None, d_lens or None, d_out_offsets or None,
                                                                       d_order or None, d_rank or None, d_bucket_offsets or None, d_bucket_widths or None, stream or None,
                                                                       C.byref(tot), C.byref(p), C.byref(cut)))
        except TkzError as ex:
            ex.needed, ex.needed_positions, ex.n_cut = tot.value, p.value, cut.value
            raise
        return tot.value, p.value, cut.value

    def bucketed_calls(self):
        """successful calls of the bucketed entries"""
        a = C.c_int64(0)
        self.lib.L.tkz_encoder_bucketed_calls(self._h, C.byref(a))
        return a.value

    # -- token-budget buckets: the sorted rows cut into buckets of at most token_budget positions (rows * width) and bucket_rows rows (tkz.h: the rule) --
    def _budgeted_host(self, fn, buf, offsets, allowed, max_len, token_budget, bucket_rows, order, bos_id, eos_id, pad_id, cut_side, pad_side, pad_multiple, want_mask, want_pos,
                       want_offs, want_rank, out_cap, bucket_cap):
        offsets = np.ascontiguousarray(offsets, dtype=np.int64)
        allowed = np.ascontiguousarray(allowed, dtype=np.int32)
        n = len(offsets) - 1
        bucket_rows = NO_ROW_CAP if bucket_rows is None else bucket_rows
        cap = (self.padded_bounds(n, max_len) if 1 <= max_len < 1 << 31 else 0) if out_cap is None else out_cap      # (a max_len out of range is refused by the library)
        bcap = n if bucket_cap is None else bucket_cap                  # (n_docs buckets always suffice)
        ids = np.empty(max(1, cap), np.int32)
        mask = np.empty(max(1, cap), np.uint8) if want_mask else None
        pos = np.empty(max(1, cap), np.int32) if want_pos else None
        lens = np.empty(max(1, n), np.int32)
        ooff = np.empty(n + 1, np.int64) if want_offs else None
        perm = np.empty(max(1, n), np.int64)
        rank = np.empty(max(1, n), np.int64) if want_rank else None
        boffs = np.empty(max(0, bcap) + 1, np.int64)
        brows = np.empty(max(0, bcap) + 1, np.int64)
        widths = np.empty(max(1, bcap), np.int32)
        tot, p, cut, nbk = C.c_int64(0), C.c_int64(0), C.c_int64(0), C.c_int64(0)
        try:
            self.lib.check(fn(self._h, buf, _ptr(offsets), n, _ptr(allowed) if len(allowed) else None, len(allowed), bos_id, eos_id, max_len, cut_side, pad_side, pad_id,
                              pad_multiple, token_budget, bucket_rows, order, _ptr(ids), cap, _ptr(mask) if want_mask else None, _ptr(pos) if want_pos else None, _ptr(lens),
                              _ptr(ooff) if want_offs else None, _ptr(perm), _ptr(rank) if want_rank else None, _ptr(boffs), _ptr(brows), _ptr(widths), bcap, C.byref(tot),
                              C.byref(p), C.byref(cut), C.byref(nbk)))
        except TkzError as ex:
            ex.needed, ex.needed_positions, ex.n_cut, ex.needed_buckets = tot.value, p.value, cut.value, nbk.value      # (E_CAPACITY: the required figures)
            raise
        P, nb = p.value, nbk.value
        return (ids[:P], mask[:P] if want_mask else None, pos[:P] if want_pos else None, lens[:n], ooff, perm[:n], rank[:n] if want_rank else None, boffs[:nb + 1],
                brows[:nb + 1], widths[:nb], tot.value, cut.value)

    def encode_batch_budgeted(self, data: np.ndarray, offsets: np.ndarray, max_len, token_budget, bucket_rows=None, order=BUCKET_ASCENDING, allowed=(), bos_id=-1, eos_id=-1,
                              pad_id=0, cut_side=TRIM_SUFFIX, pad_side=PAD_RIGHT, pad_multiple=1, want_mask=True, want_pos=True, want_offs=True, want_rank=True, out_cap=None,
                              bucket_cap=None):
        """(ids int32[P], mask uint8[P] or None, pos int32[P] or None, lens int32[n], offsets int64[n + 1] or None, order int64[n], rank int64[n] or None,
        bucket_offsets int64[n_buckets + 1], bucket_rows int64[n_buckets + 1], bucket_widths int32[n_buckets], total_tokens, n_cut): the padded rows of the documents
        sorted by len, cut greedily into buckets of at most token_budget positions (rows * width) and bucket_rows rows (None: no cap); bucket b holds the sorted rows
        bucket_rows[b] : bucket_rows[b + 1] at ids[bucket_offsets[b] : bucket_offsets[b + 1]] with its own width -- tkz_encode_batch_budgeted_utf8."""
        data = np.ascontiguousarray(data, dtype=np.uint8)
        return self._budgeted_host(self.lib.L.tkz_encode_batch_budgeted_utf8, _ptr(data) if len(data) else None, offsets, allowed, max_len, token_budget, bucket_rows, order,
                                   bos_id, eos_id, pad_id, cut_side, pad_side, pad_multiple, want_mask, want_pos, want_offs, want_rank, out_cap, bucket_cap)

    def encode_batch_budgeted_utf16(self, units: np.ndarray, offsets: np.ndarray, max_len, token_budget, bucket_rows=None, order=BUCKET_ASCENDING, allowed=(), bos_id=-1,
                                    eos_id=-1, pad_id=0, cut_side=TRIM_SUFFIX, pad_side=PAD_RIGHT, pad_multiple=1, want_mask=True, want_pos=True, want_offs=True,
                                    want_rank=True, out_cap=None, bucket_cap=None):
        """encode_batch_budgeted for UTF-16 documents (uint16[total], offsets in units) -- tkz_encode_batch_budgeted_utf16."""
        units = np.ascontiguousarray(units, dtype=np.uint16)
        buf = units if len(units) else np.zeros(1, np.uint16)
        return self._budgeted_host(self.lib.L.tkz_encode_batch_budgeted_utf16, _ptr(buf), offsets, allowed, max_len, token_budget, bucket_rows, order, bos_id, eos_id, pad_id,
                                   cut_side, pad_side, pad_multiple, want_mask, want_pos, want_offs, want_rank, out_cap, bucket_cap)

    def encode_batch_budgeted_device(self, d_bytes, d_offsets, n_docs, total_bytes, allowed, bos_id, eos_id, max_len, cut_side, pad_side, pad_id, pad_multiple, token_budget,
                                     bucket_rows, order, d_out_ids, out_cap, d_mask=0, d_pos=0, d_lens=0, d_out_offsets=0, d_order=0, d_rank=0, d_bucket_offsets=0,
                                     d_bucket_rows=0, d_bucket_widths=0, bucket_cap=0, stream=0):
        """Device buffers in and out: tkz_encode_batch_budgeted_device.  Returns (total_tokens, P, n_cut, n_buckets); a TkzError carries them as `needed`,
        `needed_positions`, `n_cut`, `needed_buckets`."""
        allowed = np.ascontiguousarray(allowed, dtype=np.int32)
        tot, p, cut, nbk = C.c_int64(0), C.c_int64(0), C.c_int64(0), C.c_int64(0)
        try:
            self.lib.check(self.lib.L.tkz_encode_batch_budgeted_device(self._h, d_bytes or None, d_offsets or None, n_docs, total_bytes, _ptr(allowed) if len(allowed) else None,
                                                                       len(allowed), bos_id, eos_id, max_len, cut_side, pad_side, pad_id, pad_multiple, token_budget,
                                                                       bucket_rows, order, d_out_ids or None, out_cap, d_mask or None, d_pos or None, d_lens or None,
                                                                       d_out_offsets or None, d_order or None, d_rank or None, d_bucket_offsets or None, d_bucket_rows or None,
                                                                       d_bucket_widths or None, bucket_cap, stream or None, C.byref(tot), C.byref(p), C.byref(cut),
                                                                       C.byref(nbk)))
        except TkzError as ex:
            ex.needed, ex.needed_positions, ex.n_cut, ex.needed_buckets = tot.value, p.value, cut.value, nbk.value
            raise
        return tot.value, p.value, cut.value, nbk.value

    def budgeted_calls(self):
        """successful calls of the budgeted entries"""
        a = C.c_int64(0)
        self.lib.L.tkz_encoder_budgeted_calls(self._h, C.byref(a))
        return a.value

    # -- pair rows: documents 2p and 2p + 1 as the two texts of row p, cut to max_len by a strategy, [bos] A sep x s B [eos], padded to the common width (tkz.h: the rule) --
    @staticmethod
    def pairs_bounds(n_pairs, max_len):
        """the ids (and mask and type bytes, and pos entries) that always suffice (tkz.h): a row of max_len a pair"""
        return n_pairs * max_len

    def _pairs_host(self, fn, buf, offsets, allowed, max_len, bos_id, sep_id, sep_count, eos_id, pad_id, strategy, cut_side, pad_side, pad_multiple, want_mask, want_types,
                    want_pos, want_kept, want_offs, out_cap):
        offsets = np.ascontiguousarray(offsets, dtype=np.int64)
        allowed = np.ascontiguousarray(allowed, dtype=np.int32)
        n = len(offsets) - 1
        npairs = n // 2
        cap = (self.pairs_bounds(npairs, max_len) if 1 <= max_len < 1 << 31 else 0) if out_cap is None else out_cap      # (a max_len out of range is refused by the library)
        ids = np.empty(max(1, cap), np.int32)
        mask = np.empty(max(1, cap), np.uint8) if want_mask else None
        types = np.empty(max(1, cap), np.uint8) if want_types else None
        pos = np.empty(max(1, cap), np.int32) if want_pos else None
        lens = np.empty(max(1, npairs), np.int32)
        kept = np.empty(max(1, n), np.int32) if want_kept else None
        ooff = np.empty(n + 1, np.int64) if want_offs else None
        tot, w, cut = C.c_int64(0), C.c_int64(0), C.c_int64(0)
        try:
            self.lib.check(fn(self._h, buf, _ptr(offsets), n, _ptr(allowed) if len(allowed) else None, len(allowed), bos_id, sep_id, sep_count, eos_id, max_len, strategy,
                              cut_side, pad_side, pad_id, pad_multiple, _ptr(ids), cap, _ptr(mask) if want_mask else None, _ptr(types) if want_types else None,
                              _ptr(pos) if want_pos else None, _ptr(lens), _ptr(kept) if want_kept else None, _ptr(ooff) if want_offs else None,
                              C.byref(tot), C.byref(w), C.byref(cut)))
        except TkzError as ex:
            ex.needed, ex.needed_width, ex.n_cut = tot.value, w.value, cut.value      # (E_CAPACITY: the required figures)
            raise
        W = w.value
        rows = lambda a: a[:npairs * W].reshape(npairs, W)
        return (rows(ids), rows(mask) if want_mask else None, rows(types) if want_types else None, rows(pos) if want_pos else None, lens[:npairs],
                kept[:2 * npairs].reshape(npairs, 2) if want_kept else None, ooff, tot.value, cut.value)

    def encode_batch_pairs(self, data: np.ndarray, offsets: np.ndarray, max_len, allowed=(), bos_id=-1, sep_id=-1, sep_count=0, eos_id=-1, pad_id=0, strategy=TRUNC_LONGEST_FIRST,
                           cut_side=TRIM_SUFFIX, pad_side=PAD_RIGHT, pad_multiple=1, want_mask=True, want_types=True, want_pos=True, want_kept=True, want_offs=True, out_cap=None):
        """(ids int32[n_pairs, W], mask uint8[n_pairs, W] or None, type_ids uint8[n_pairs, W] or None, pos int32[n_pairs, W] or None, lens int32[n_pairs],
        kept int32[n_pairs, 2] or None, offsets int64[n_docs + 1] or None, total_tokens, n_cut): documents 2p and 2p + 1 are the two texts of pair p; the ids of
        encode_batch / encode_batch_special cut to max_len by the strategy, framed, joined and padded to the common width W -- tkz_encode_batch_pairs_utf8."""
        data = np.ascontiguousarray(data, dtype=np.uint8)
        return self._pairs_host(self.lib.L.tkz_encode_batch_pairs_utf8, _ptr(data) if len(data) else None, offsets, allowed, max_len, bos_id, sep_id, sep_count, eos_id, pad_id,
                                strategy, cut_side, pad_side, pad_multiple, want_mask, want_types, want_pos, want_kept, want_offs, out_cap)

    def encode_batch_pairs_utf16(self, units: np.ndarray, offsets: np.ndarray, max_len, allowed=(), bos_id=-1, sep_id=-1, sep_count=0, eos_id=-1, pad_id=0,
                                 strategy=TRUNC_LONGEST_FIRST, cut_side=TRIM_SUFFIX, pad_side=PAD_RIGHT, pad_multiple=1, want_mask=True, want_types=True, want_pos=True,
                                 want_kept=True, want_offs=True, out_cap=None):
        """encode_batch_pairs for UTF-16 documents (uint16[total], offsets in units) -- tkz_encode_batch_pairs_utf16."""
        units = np.ascontiguousarray(units, dtype=np.uint16)
        buf = units if len(units) else np.zeros(1, np.uint16)
        return self._pairs_host(self.lib.L.tkz_encode_batch_pairs_utf16, _ptr(buf), offsets, allowed, max_len, bos_id, sep_id, sep_count, eos_id, pad_id, strategy, cut_side,
                                pad_side, pad_multiple, want_mask, want_types, want_pos, want_kept, want_offs, out_cap)

    def encode_batch_pairs_device(self, d_bytes, d_offsets, n_docs, total_bytes, allowed, bos_id, sep_id, sep_count, eos_id, max_len, strategy, cut_side, pad_side, pad_id,
                                  pad_multiple, d_out_ids, out_cap, d_mask=0, d_type_ids=0, d_pos=0, d_lens=0, d_kept=0, d_out_offsets=0, stream=0):
        """Device buffers in and out: tkz_encode_batch_pairs_device.  Returns (total_tokens, W, n_cut); a TkzError carries them as `needed`, `needed_width`, `n_cut`."""
        allowed = np.ascontiguousarray(allowed, dtype=np.int32)
        tot, w, cut = C.c_int64(0), C.c_int64(0), C.c_int64(0)
        try:
            self.lib.check(self.lib.L.tkz_encode_batch_pairs_device(self._h, d_bytes or None, d_offsets or None, n_docs, total_bytes, _ptr(allowed) if len(allowed) else None,
                                                                    len(allowed), bos_id, sep_id, sep_count, eos_id, max_len, strategy, cut_side, pad_side, pad_id, pad_multiple,
                                                                    d_out_ids or None, out_cap, d_mask or None, d_type_ids or None, d_pos or None, d_lens or None,
                                                                    d_kept or None, d_out_offsets or None, stream or None, C.byref(tot), C.byref(w), C.byref(cut)))
        except TkzError as ex:
            ex.needed, ex.needed_width, ex.n_cut = tot.value, w.value, cut.value
            raise
        return tot.value, w.value, cut.value

    def pairs_calls(self):
        """successful calls of the pair entries"""
        a = C.c_int64(0)
        self.lib.L.tkz_encoder_pairs_calls(self._h, C.byref(a))
        return a.value

    def set_special_tokens(self, specials):
        """specials: {literal str: id}.  Registers SpecialTokensDecoder for Decode (TikTokenizer.cs:79) and, in this order, the literals the special
        entries cut out of the text (encode_batch_special)."""
        items = list(specials.items())
        lits = [k.encode("utf-8") for k, _ in items]
        ids = np.asarray([v for _, v in items], dtype=np.int32)
        blob = np.frombuffer(b"".join(lits), np.uint8) if sum(map(len, lits)) else np.zeros(1, np.uint8)
        offs = np.cumsum([0] + [len(x) for x in lits]).astype(np.int64)
        self.lib.check(self.lib.L.tkz_encoder_set_special_tokens(self._h, _ptr(ids) if len(ids) else None, _ptr(blob), _ptr(offs), len(ids)))

    def decode_batch(self, ids: np.ndarray, id_offsets: np.ndarray, out_cap=None):
        """Batch Decode on the device: (bytes uint8[total], byte_offsets int64[n+1])."""
        ids = np.ascontiguousarray(ids, dtype=np.int32)
        id_offsets = np.ascontiguousarray(id_offsets, dtype=np.int64)
        n = len(id_offsets) - 1
        cap = out_cap if out_cap is not None else max(16, 8 * len(ids))
        while True:
            out = np.empty(max(1, cap), np.uint8)
            ooff = np.empty(n + 1, np.int64)
            needed = C.c_int64(0)
            st = self.lib.L.tkz_decode_batch(self._h, _ptr(ids) if len(ids) else None, _ptr(id_offsets), n, _ptr(out), cap, _ptr(ooff), C.byref(needed))
            if st == E_CAPACITY and out_cap is None:
                cap = needed.value
                continue
            self.lib.check(st)
            return out[:needed.value], ooff

    def decode_batch_device(self, d_ids, d_id_offsets, n_docs, total_ids, d_out, out_cap, d_out_offsets, stream=0):
        tot = C.c_int64(0)
        self.lib.check(self.lib.L.tkz_decode_batch_device(self._h, d_ids, d_id_offsets, n_docs, total_ids, d_out, out_cap, d_out_offsets,
                                                          stream or None, C.byref(tot)))
        return tot.value

    def decode_batch_utf16(self, ids: np.ndarray, id_offsets: np.ndarray, out_cap=None):
        """Batch Decode to UTF-16 on the device (Encoding.UTF8.GetString of every document): (units uint16[total], unit_offsets int64[n+1])."""
        ids = np.ascontiguousarray(ids, dtype=np.int32)
        id_offsets = np.ascontiguousarray(id_offsets, dtype=np.int64)
        n = len(id_offsets) - 1
        cap = out_cap if out_cap is not None else max(16, 8 * len(ids))
        while True:
            out = np.empty(max(1, cap), np.uint16)
            ooff = np.empty(n + 1, np.int64)
            needed = C.c_int64(0)
            st = self.lib.L.tkz_decode_batch_utf16(self._h, _ptr(ids) if len(ids) else None, _ptr(id_offsets), n, _ptr(out), cap, _ptr(ooff), C.byref(needed))
            if st == E_CAPACITY and out_cap is None:
                cap = needed.value
                continue
            self.lib.check(st)
            return out[:needed.value], ooff

    def _decode_one(self, fn, dtype, ids, out_cap):
        ids = np.ascontiguousarray(ids, dtype=np.int32)
        cap = out_cap if out_cap is not None else max(16, 8 * len(ids))
        while True:
            out = np.empty(max(1, cap), dtype)
            n = C.c_int64(0)
            st = fn(self._h, _ptr(ids) if len(ids) else None, len(ids), _ptr(out), cap, C.byref(n))
            if st == E_CAPACITY and out_cap is None:
                cap = n.value
                continue
            self.lib.check(st)
            return out[:n.value]

    def decode(self, ids: np.ndarray, out_cap=None):
        """Decode of ONE id list (tkz_decode_utf8: a single launch for a list of up to 32,768 ids): bytes uint8[total]."""
        return self._decode_one(self.lib.L.tkz_decode_utf8, np.uint8, ids, out_cap)

    def decode_utf16(self, ids: np.ndarray, out_cap=None):
        """The same to UTF-16 (tkz_decode_utf16): units uint16[total]."""
        return self._decode_one(self.lib.L.tkz_decode_utf16, np.uint16, ids, out_cap)

    def decode_batch_utf16_device(self, d_ids, d_id_offsets, n_docs, total_ids, d_out, out_cap, d_out_offsets, stream=0):
        tot = C.c_int64(0)
        self.lib.check(self.lib.L.tkz_decode_batch_utf16_device(self._h, d_ids, d_id_offsets, n_docs, total_ids, d_out, out_cap, d_out_offsets,
                                                                stream or None, C.byref(tot)))
        return tot.value

    @property
    def counts_device(self):
        """Device pointer to {n_docs, n_bytes, n_tokens} (3 int64) of the last batch."""
        return self.lib.L.tkz_encoder_counts_device(self._h)

    # -- device buffers (raw pointers, e.g. torch tensors' data_ptr()) --
    def encode_batch_device(self, d_bytes, d_offsets, n_docs, total_bytes, d_out_ids, out_cap, d_out_offsets, stream=0):
        tot = C.c_int64(0)
        self.lib.check(self.lib.L.tkz_encode_batch_device(self._h, d_bytes, d_offsets, n_docs, total_bytes, d_out_ids, out_cap,
                                                          d_out_offsets, stream or None, C.byref(tot)))
        return tot.value

    def encode_batch_device_begin(self, d_bytes, d_offsets, n_docs, total_bytes, d_out_ids, out_cap, d_out_offsets, stream=0, d_counts3=0):
        """Enqueues the batch and returns a handle for encode_batch_device_end (several may be in flight).  d_counts3: device pointer to
        3 int64 of the caller's that receive THIS batch's {n_docs, n_bytes, n_tokens} (final once _end has returned)."""
        h = C.c_void_p()
        self.lib.check(self.lib.L.tkz_encode_batch_device_begin_counts(self._h, d_bytes, d_offsets, n_docs, total_bytes, d_out_ids, out_cap,
                                                                       d_out_offsets, stream or None, d_counts3 or None, C.byref(h)))
        return h

    def pending_counts_device(self, pending):
        """Device pointer to the {n_docs, n_bytes, n_tokens} block of a batch in flight (tkz_pending_counts_device)."""
        return self.lib.L.tkz_pending_counts_device(pending)

    def encode_batch_device_end(self, pending):
        tot = C.c_int64(0)
        self.lib.check(self.lib.L.tkz_encode_batch_device_end(pending, C.byref(tot)))
        return tot.value


class Comm:
    """The direct-RCCL communicator of the C ABI (tkz_comm_*): one all-gather of {n_docs, n_bytes, n_tokens} per batch.
    `exchange(id_or_None) -> id`: how the 128-byte id travels from rank 0 to the others (any broadcast the host has)."""

    ID_BYTES = 128

    def __init__(self, rank: int, world: int, device: int, exchange, lib: Library = None):
        self.lib = lib or default_library()
        if not self.lib.has_comm:
            raise RuntimeError("this build of libtkz has no communicator")
        idbuf = (C.c_uint8 * self.ID_BYTES)()
        if rank == 0:
            self.lib.check(self.lib.L.tkz_comm_unique_id(idbuf))
        got = exchange(bytes(idbuf) if rank == 0 else None)
        assert len(got) == self.ID_BYTES
        idbuf = (C.c_uint8 * self.ID_BYTES).from_buffer_copy(got)
        h = C.c_void_p()
        self.lib.check(self.lib.L.tkz_comm_create(idbuf, rank, world, device, C.byref(h)))
        self._h = h

    def __del__(self):
        self.close()

    def close(self):
        if getattr(self, "_h", None):
            self.lib.L.tkz_comm_destroy(self._h)
            self._h = None

    @property
    def world(self):
        return self.lib.L.tkz_comm_world(self._h)

    @property
    def rank(self):
        return self.lib.L.tkz_comm_rank(self._h)

    @property
    def backend(self):
        return self.lib.L.tkz_comm_backend(self._h).decode()

    def allgather_counts_device(self, d_mine, d_table, stream=0):
        """d_mine: device pointer to 3 int64 (Encoder.counts_device); d_table: device pointer to world*3 int64.  Asynchronous."""
        self.lib.check(self.lib.L.tkz_comm_allgather_counts_device(self._h, d_mine, d_table, stream or None))

    def allgather_counts(self, n_docs, n_bytes, n_tokens):
        table = np.zeros(self.world * 3, np.int64)
        self.lib.check(self.lib.L.tkz_comm_allgather_counts(self._h, n_docs, n_bytes, n_tokens, table.ctypes.data))
        return table.reshape(self.world, 3)


def shard_range(n_docs_total, rank, world, lib: Library = None):
    lib = lib or default_library()
    lo, hi = C.c_int64(0), C.c_int64(0)
    lib.L.tkz_shard_range(n_docs_total, rank, world, C.byref(lo), C.byref(hi))
    return lo.value, hi.value


def shard_bases(table, rank, lib: Library = None):
    """table: int64[world, 3] as gathered.  Returns (bases3, totals3) as lists {docs, bytes, tokens}."""
    lib = lib or default_library()
    t = np.ascontiguousarray(table, dtype=np.int64).reshape(-1, 3)
    b, tot = np.zeros(3, np.int64), np.zeros(3, np.int64)
    lib.check(lib.L.tkz_shard_bases(t.ctypes.data, len(t), rank, b.ctypes.data, tot.ctypes.data))
    return b.tolist(), tot.tolist()


def shard_write(path, ids, offsets, doc_base=0, token_base=0, lib: Library = None):
    """tkz_shard_write on host arrays."""
    lib = lib or default_library()
    ids = np.ascontiguousarray(ids, dtype=np.int32)
    offsets = np.ascontiguousarray(offsets, dtype=np.int64)
    lib.check(lib.L.tkz_shard_write(os.fsencode(path), _ptr(ids) if len(ids) else None, len(ids), _ptr(offsets), len(offsets) - 1, doc_base, token_base))


def shard_write_device(path, d_ids, n_tokens, d_offsets, n_docs, doc_base=0, token_base=0, device=0, lib: Library = None):
    """tkz_shard_write_device: straight from HBM (raw device pointers)."""
    lib = lib or default_library()
    lib.check(lib.L.tkz_shard_write_device(os.fsencode(path), device, d_ids, n_tokens, d_offsets, n_docs, doc_base, token_base))


def shard_read_header(path, lib: Library = None):
    lib = lib or default_library()
    v = [C.c_int64(0) for _ in range(4)]
    lib.check(lib.L.tkz_shard_read_header(os.fsencode(path), *[C.byref(x) for x in v]))
    return tuple(x.value for x in v)      # n_docs, n_tokens, doc_base, token_base


def corpus_doc_host(kind, seed, doc_index, min_len, max_len, lib: Library = None) -> bytes:
    lib = lib or default_library()
    n = lib.L.tkz_corpus_generate_doc_host(kind, seed, doc_index, min_len, max_len, None, 0)
    buf = np.zeros(max(1, n), np.uint8)
    lib.L.tkz_corpus_generate_doc_host(kind, seed, doc_index, min_len, max_len, buf.ctypes.data, n)
    return buf[:n].tobytes()


def corpus_generate_device(device, kind, seed, first_doc, n_docs, min_len, max_len, d_offsets, d_bytes, cap_bytes, stream=0,
                           lib: Library = None):
    lib = lib or default_library()
    tot = C.c_int64(0)
    lib.check(lib.L.tkz_corpus_generate_device(device, kind, seed, first_doc, n_docs, min_len, max_len, d_offsets, d_bytes or None,
                                               cap_bytes, stream or None, C.byref(tot)))
    return tot.value
