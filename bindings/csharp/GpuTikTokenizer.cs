// GpuTikTokenizer.cs -- ITokenizer over libtkz (MI355X).  SOURCE ONLY: the build image has no .NET toolchain
// (no dotnet / mono / csc), so this file is not compiled or tested here; the same boundary is exercised through
// ctypes (tokenizer_amd/_native.py) and C++ (include/tkz_tokenizer.hpp).  See INTEGRATION.md.
//
// Written against what the reference's project gives it: netstandard2.0, LangVersion 8.0, Nullable enable, no package
// references beyond the BCL (TokenizerLib.csproj:4-5,10) plus <AllowUnsafeBlocks>.  So: no System.Memory (no Span, no
// AsSpan, no Encoding overloads over spans -- the char* / byte* overloads instead), no System.Range / System.Index (Substring,
// not text[a..b]), no Marshal.PtrToStringUTF8 and no UnmanagedType.LPUTF8Str (UTF-8 strings cross the boundary as byte[]).
// INTEGRATION.md lists every BCL member used with where it comes from.
//
// Drop it into Tokenizer_C#/TokenizerLib next to TikTokenizer.cs.  It keeps the two Encode overloads of
// ITokenizer (ITokenizer.cs:12,28) and adds EncodeBatch; special-token segmentation is the reference's own
// EncodeInternal / FindNextSpecialToken (TikTokenizer.cs:141-170,230-241) with the plain segments sent to the
// GPU in one batch.  The trim variants (TikTokenizer.cs:288-579) get the token count and length of every regex piece
// from tkz_encode_batch_pieces_utf8 and decide the cut on the host; Decode / DecodeBatch run on the device too
// (tkz_decode_batch_utf16: the code units of every string come from the device, Encoding.UTF8.GetString included).  ShardedEncoder at the end is the multi-GPU form: one process per GPU, contiguous document
// ranges, ONE RCCL all-gather of the per-rank counts through libtkz's own communicator (tkz_comm_*), token shard files.
using System;
using System.Collections.Generic;
using System.IO;
using System.Linq;
using System.Runtime.InteropServices;
using System.Text;
using System.Text.RegularExpressions;

namespace Microsoft.DeepDev
{
    internal static class Tkz
    {
        private const string Lib = "tkz";   // libtkz.so

        [DllImport(Lib)] internal static extern IntPtr tkz_last_error();
        [DllImport(Lib)] internal static extern int tkz_vocab_from_tiktoken(byte[] file, UIntPtr n, out IntPtr vocab);
        [DllImport(Lib)] internal static extern void tkz_vocab_destroy(IntPtr vocab);
        [DllImport(Lib)] internal static extern int tkz_pattern_from_regex(byte[] regexUtf8Z, out int pattern);   // .NET semantics (TikTokenizer.cs:77): the o200k string gives TKZ_PATTERN_O200K_DOTNET
        [DllImport(Lib)] internal static extern int tkz_encoder_create(IntPtr vocab, int pattern, int device, out IntPtr encoder);
        [DllImport(Lib)] internal static extern int tkz_encoder_set_option(IntPtr encoder, int option, long value);
        [DllImport(Lib)] internal static extern int tkz_encoder_reserve(IntPtr encoder, long maxBytes, long maxDocs);   // the workspace of batches up to that size, allocated now (TokenizerBuilder.cs:210-213: construction pays, not the first Encode)
        [DllImport(Lib)] internal static extern int tkz_encoder_set_unicode_classes(IntPtr encoder, byte[] classes, long nCodePoints);   // the HOST's Unicode classification (TikTokenizer.cs:77: the running process's regex engine defines the split)
        [DllImport(Lib)] internal static extern int tkz_host_alloc(UIntPtr bytes, out IntPtr p);        // page-locked memory: copies to and from it run at the PCIe rate
        [DllImport(Lib)] internal static extern void tkz_host_free(IntPtr p);
        [DllImport(Lib)] internal static extern void tkz_encoder_destroy(IntPtr encoder);
        [DllImport(Lib)] internal static extern unsafe int tkz_encode_batch_utf8(IntPtr encoder, byte* bytes, long* docOffsets, long nDocs,
                                                                                  int* outIds, long outCap, long* outOffsets, out long needed);
        [DllImport(Lib)] internal static extern unsafe int tkz_encode_utf16(IntPtr encoder, char* text, long len, int* outIds, long outCap, out long nOut);
        [DllImport(Lib)] internal static extern unsafe int tkz_encode_special_utf16(IntPtr encoder, char* text, long len, int* allowed, int nAllowed, int* outIds, long outCap, out long nOut);
        // EncodeTrimSuffix / EncodeTrimPrefix on ONE string: one kernel launch for a prompt (include/tkz.h).  (Like the rest of this file: not compiled here.)
        [DllImport(Lib)] internal static extern unsafe int tkz_encode_trim_utf16(IntPtr encoder, char* text, long len, int* allowed, int nAllowed, int side, long maxTokens,
                                                                                  int* outIds, long outCap, out long nOut, out long cutUnits);
        [DllImport(Lib)] internal static extern unsafe int tkz_encode_batch_utf16(IntPtr encoder, char* units, long* unitOffsets, long nDocs,
                                                                                   int* outIds, long outCap, long* outOffsets, out long needed);
        [DllImport(Lib)] internal static extern unsafe int tkz_encoder_set_special_tokens(IntPtr encoder, int* ids, byte* literalsUtf8, long* literalOffsets, int n);
        [DllImport(Lib)] internal static extern unsafe int tkz_decode_batch(IntPtr encoder, int* ids, long* idOffsets, long nDocs, byte* outBytes, long outCap, long* outOffsets, out long needed);
        [DllImport(Lib)] internal static extern unsafe int tkz_decode_batch_utf16(IntPtr encoder, int* ids, long* idOffsets, long nDocs, char* outUnits, long outCap, long* outOffsets, out long needed);
        // Decode(int[]) of ONE id list: one kernel launch for up to 32,768 ids (include/tkz.h).  (Like the rest of this file: not compiled here.)
        [DllImport(Lib)] internal static extern unsafe int tkz_decode_utf16(IntPtr encoder, int* ids, long nIds, char* outUnits, long outCap, out long nOut);
        [DllImport(Lib)] internal static extern void tkz_encoder_small_decode_calls(IntPtr encoder, out long calls, out long handedBack);
        // Encode(...).Count without the ids: the token offsets (or the one count) come back, no id buffer exists
        [DllImport(Lib)] internal static extern unsafe int tkz_count_utf16(IntPtr encoder, char* text, long len, int* allowed, int nAllowed, out long nOut);
        [DllImport(Lib)] internal static extern unsafe int tkz_count_batch_utf16(IntPtr encoder, char* units, long* unitOffsets, long nDocs, int* allowed, int nAllowed,
                                                                                  long* outOffsets, out long totalTokens);
        [DllImport(Lib)] internal static extern void tkz_encoder_count_calls(IntPtr encoder, out long calls, out long singleLaunch);
        // token spans: Encode, and where every token's text starts in the string, in code units (include/tkz.h, "Token spans")
        [DllImport(Lib)] internal static extern unsafe int tkz_encode_batch_spans_utf16(IntPtr encoder, char* units, long* unitOffsets, long nDocs, int* allowed, int nAllowed,
                                                                                         int* outIds, long outCap, long* outOffsets, int* tokUnits, out long needed);
        [DllImport(Lib)] internal static extern void tkz_encoder_spans_calls(IntPtr encoder, out long calls);
        // token-budget chunks: Encode, and the tokens of every text cut into chunks of at most maxTokens (include/tkz.h, "Token-budget chunks")
        [DllImport(Lib)] internal static extern unsafe int tkz_encode_batch_chunks_utf16(IntPtr encoder, char* units, long* unitOffsets, long nDocs, int* allowed, int nAllowed,
                                                                                          long maxTokens, int* outIds, long outCap, long* outOffsets, long* docChunkOffsets,
                                                                                          long* chunkTokens, long* chunkUnits, long chunkCap, out long neededIds, out long neededChunks);
        [DllImport(Lib)] internal static extern void tkz_encoder_chunks_calls(IntPtr encoder, out long calls);
        // overlapping token-budget chunks: a chunk size and an overlap, a start and an end a chunk (include/tkz.h, "Overlapping token-budget chunks")
        [DllImport(Lib)] internal static extern unsafe int tkz_encode_batch_chunks_overlap_utf16(IntPtr encoder, char* units, long* unitOffsets, long nDocs, int* allowed, int nAllowed,
                                                                                                  long maxTokens, long overlap, int* outIds, long outCap, long* outOffsets,
                                                                                                  long* docChunkOffsets, long* chunkTokens, long* chunkEnds, long* chunkUnits,
                                                                                                  long* chunkEndUnits, long chunkCap, out long neededIds, out long neededChunks);
        [DllImport(Lib)] internal static extern void tkz_encoder_chunks_overlap_calls(IntPtr encoder, out long calls);
        // packed rows: Encode's ids framed by bos / eos ids, in rows of the context length, with positions and segment starts (include/tkz.h, "Packed rows")
        [DllImport(Lib)] internal static extern unsafe int tkz_encode_batch_packed_utf16(IntPtr encoder, char* units, long* unitOffsets, long nDocs, int* allowed, int nAllowed,
                                                                                          int bosId, int eosId, long rowLen, int padId, int* outIds, long outCap, long* outOffsets,
                                                                                          int* pos, long* segStarts, long segCap, out long totalTokens, out long neededIds, out long neededSegs);
        [DllImport(Lib)] internal static extern void tkz_encoder_packed_calls(IntPtr encoder, out long calls);
        // padded rows: Encode's ids cut to a maximum length, framed by bos / eos ids, a row a text padded to a common width, with the mask, pos and lens (include/tkz.h, "Padded rows")
        [DllImport(Lib)] internal static extern unsafe int tkz_encode_batch_padded_utf16(IntPtr encoder, char* units, long* unitOffsets, long nDocs, int* allowed, int nAllowed,
                                                                                          int bosId, int eosId, long maxLen, int cutSide, int padSide, int padId, long padMultiple,
                                                                                          int* outIds, long outCap, byte* mask, int* pos, int* lens, long* outOffsets,
                                                                                          out long totalTokens, out long width, out long nCut);
        [DllImport(Lib)] internal static extern void tkz_encoder_padded_calls(IntPtr encoder, out long calls);
        // length-bucketed padded rows: the padded rows of the texts sorted by length, every bucket of bucketRows rows at its own width (include/tkz.h, "Length-bucketed padded rows")
        [DllImport(Lib)] internal static extern unsafe int tkz_encode_batch_bucketed_utf16(IntPtr encoder, char* units, long* unitOffsets, long nDocs, int* allowed, int nAllowed,
                                                                                            int bosId, int eosId, long maxLen, int cutSide, int padSide, int padId, long padMultiple,
                                                                                            long bucketRows, int order, int* outIds, long outCap, byte* mask, int* pos, int* lens,
                                                                                            long* outOffsets, long* orderOut, long* rank, long* bucketOffsets, int* bucketWidths,
                                                                                            out long totalTokens, out long totalPositions, out long nCut);
        [DllImport(Lib)] internal static extern void tkz_encoder_bucketed_calls(IntPtr encoder, out long calls);
        // token-budget buckets: the same sorted rows cut into buckets of at most tokenBudget positions (rows x width) and bucketRows rows (include/tkz.h, "Token-budget buckets")
        [DllImport(Lib)] internal static extern unsafe int tkz_encode_batch_budgeted_utf16(IntPtr encoder, char* units, long* unitOffsets, long nDocs, int* allowed, int nAllowed,
                                                                                            int bosId, int eosId, long maxLen, int cutSide, int padSide, int padId, long padMultiple,
                                                                                            long tokenBudget, long bucketRows, int order, int* outIds, long outCap, byte* mask, int* pos,
                                                                                            int* lens, long* outOffsets, long* orderOut, long* rank, long* bucketOffsets,
                                                                                            long* bucketRowsOut, int* bucketWidths, long bucketCap, out long totalTokens,
                                                                                            out long totalPositions, out long nCut, out long nBuckets);
        [DllImport(Lib)] internal static extern void tkz_encoder_budgeted_calls(IntPtr encoder, out long calls);
        // pair rows: two texts a row -- [bos] A sep B [eos] --, cut to a maximum length by a strategy, padded to a common width, with the mask, the type ids, pos, lens and the kept counts (include/tkz.h, "Pair rows")
        [DllImport(Lib)] internal static extern unsafe int tkz_encode_batch_pairs_utf16(IntPtr encoder, char* units, long* unitOffsets, long nDocs, int* allowed, int nAllowed,
                                                                                         int bosId, int sepId, int sepCount, int eosId, long maxLen, int strategy, int cutSide, int padSide,
                                                                                         int padId, long padMultiple, int* outIds, long outCap, byte* mask, byte* typeIds, int* pos, int* lens,
                                                                                         int* kept, long* outOffsets, out long totalTokens, out long width, out long nCut);
        [DllImport(Lib)] internal static extern void tkz_encoder_pairs_calls(IntPtr encoder, out long calls);
        // multi-GPU: the count exchange and the shard arithmetic (include/tkz.h, "multi-GPU"), token shard files
        [DllImport(Lib)] internal static extern int tkz_comm_unique_id(byte[] id128);
        [DllImport(Lib)] internal static extern int tkz_comm_create(byte[] id128, int rank, int world, int device, out IntPtr comm);
        [DllImport(Lib)] internal static extern void tkz_comm_destroy(IntPtr comm);
        [DllImport(Lib)] internal static extern int tkz_comm_world(IntPtr comm);
        [DllImport(Lib)] internal static extern int tkz_comm_allgather_counts(IntPtr comm, long nDocs, long nBytes, long nTokens, long[] table);
        [DllImport(Lib)] internal static extern void tkz_shard_range(long nDocsTotal, int rank, int world, out long lo, out long hi);
        [DllImport(Lib)] internal static extern int tkz_shard_bases(long[] table, int world, int rank, long[] bases3, long[] totals3);
        [DllImport(Lib)] internal static extern int tkz_shard_write(byte[] pathUtf8Z, int[] ids, long nTokens, long[] offsets, long nDocs, long docBase, long tokenBase);
        [DllImport(Lib)] internal static extern unsafe int tkz_encode_batch_pieces_utf8(IntPtr encoder, byte* bytes, long* docOffsets, long nDocs, int* outIds, long outCap,
                                                                                         long* docPieceOffsets, long* pieceByteOffsets, long* pieceTokenOffsets,
                                                                                         long pieceCap, out long nPieces, out long neededIds);
        // EncodeTrimSuffix / EncodeTrimPrefix for a batch, cut on the device (include/tkz.h).  tkz_encode_batch_trim_device is for hosts that hold their text in HBM;
        // the class uses the host-buffer entry.  (Like the rest of this file: not compiled here.)
        [DllImport(Lib)] internal static extern unsafe int tkz_encode_batch_trim_device(IntPtr encoder, IntPtr dBytes, IntPtr dDocOffsets, long nDocs, long totalBytes,
                                                                                         int* allowed, int nAllowed, int side, long maxTokens, IntPtr dMaxTokens,
                                                                                         IntPtr dOutIds, long outCap, IntPtr dOutOffsets, IntPtr dCutBytes, IntPtr dCutUnits,
                                                                                         IntPtr hipStream, out long totalTokens);
        // Encode(text, allowedSpecial) / EncodeTrimSuffix / EncodeTrimPrefix on a batch of strings' own chars: the device transcodes, and searches the literals as
        // .NET searches the string (a lone surrogate is not U+FFFD).  (Like the rest of this file: not compiled here.)
        [DllImport(Lib)] internal static extern unsafe int tkz_encode_batch_special_utf16(IntPtr encoder, char* units, long* unitOffsets, long nDocs, int* allowed, int nAllowed,
                                                                                         int* outIds, long outCap, long* outOffsets, out long needed);
        [DllImport(Lib)] internal static extern unsafe int tkz_encode_batch_trim_utf16(IntPtr encoder, char* units, long* unitOffsets, long nDocs, int* allowed, int nAllowed,
                                                                                      int side, long maxTokens, long* maxTokensPerDoc, int* outIds, long outCap, long* outOffsets,
                                                                                      long* cutUnits, out long needed);
        [DllImport(Lib)] internal static extern unsafe int tkz_encode_batch_trim_utf8(IntPtr encoder, byte* bytes, long* docOffsets, long nDocs, int* allowed, int nAllowed,
                                                                                       int side, long maxTokens, long* maxTokensPerDoc, int* outIds, long outCap, long* outOffsets,
                                                                                       long* cutBytes, long* cutUnits, out long needed);

        /// <summary>A C string argument: the UTF-8 bytes and a terminating zero.</summary>
        internal static byte[] Utf8Z(string s)
        {
            var b = new byte[Encoding.UTF8.GetByteCount(s) + 1];
            Encoding.UTF8.GetBytes(s, 0, s.Length, b, 0);
            return b;
        }

        /// <summary>A zero-terminated UTF-8 string owned by the library (tkz_last_error).</summary>
        internal static string Utf8ToString(IntPtr p)
        {
            if (p == IntPtr.Zero) return "";
            int n = 0;
            while (Marshal.ReadByte(p, n) != 0) ++n;
            var b = new byte[n];
            Marshal.Copy(p, b, 0, n);
            return Encoding.UTF8.GetString(b, 0, n);
        }

        internal static void Check(int status)
        {
            if (status == 0) return;
            string msg = Utf8ToString(tkz_last_error());
            switch (status)
            {
                case -1: throw new InvalidOperationException("Failed to load from BPE encoder file stream: " + msg, new FormatException(msg));  // TikTokenizer.cs:133-136
                case -2: throw new ArgumentException(msg);                    // TikTokenizer.cs:84-87
                case -3: throw new KeyNotFoundException(msg);                 // BytePairEncoder.cs:17,73
                case -7: throw new NotImplementedException(msg);              // TokenizerBuilder.cs:179
                case -9: throw new PlatformNotSupportedException(msg);        // no HIP device: there is no CPU fallback in libtkz
                case -10: throw new OutOfMemoryException(msg);                // device memory for the workspace
                default: throw new InvalidOperationException("libtkz status " + status + ": " + msg);
            }
        }
    }

    /// <summary>The native encoder (device tables + workspaces): released exactly once, also when Dispose is never called.</summary>
    internal sealed class EncoderHandle : SafeHandle
    {
        public EncoderHandle(IntPtr h) : base(IntPtr.Zero, true) { SetHandle(h); }
        public override bool IsInvalid => handle == IntPtr.Zero;
        protected override bool ReleaseHandle() { Tkz.tkz_encoder_destroy(handle); return true; }
    }

    /// <summary>Two grow-only page-locked buffers (tkz_host_alloc): the code units on their way to the device, the ids on their way back.  A tokenizer
    /// keeps a pool of these sets; every EncodeBatchFlat in flight rents its own (two for a batch that goes in sub-batches) and returns them.</summary>
    internal sealed class PinnedBuffers : IDisposable
    {
        private IntPtr units, ids; private long unitsCap, idsCap;
        private static IntPtr Ensure(ref IntPtr p, ref long cap, long bytes)
        {
            if (bytes > cap)
            {
                if (p != IntPtr.Zero) Tkz.tkz_host_free(p);
                p = IntPtr.Zero; cap = 0;
                long want = bytes + bytes / 4 + 4096;
                Tkz.Check(Tkz.tkz_host_alloc((UIntPtr)(ulong)want, out p));
                cap = want;
            }
            return p;
        }
        public IntPtr Units(long bytes) => Ensure(ref units, ref unitsCap, bytes);
        public IntPtr Ids(long bytes) => Ensure(ref ids, ref idsCap, bytes);
        /// <summary>A larger id buffer that still holds the first keepBytes of the old one.</summary>
        public unsafe void GrowIdsKeeping(long keepBytes, long newBytes)
        {
            if (newBytes <= idsCap) return;
            long want = newBytes + newBytes / 4 + 4096;
            Tkz.Check(Tkz.tkz_host_alloc((UIntPtr)(ulong)want, out IntPtr p));
            if (ids != IntPtr.Zero)
            {
                if (keepBytes > 0) Buffer.MemoryCopy((void*)ids, (void*)p, want, keepBytes);
                Tkz.tkz_host_free(ids);
            }
            ids = p; idsCap = want;
        }
        public void Dispose()
        {
            if (units != IntPtr.Zero) Tkz.tkz_host_free(units);
            if (ids != IntPtr.Zero) Tkz.tkz_host_free(ids);
            units = ids = IntPtr.Zero; unitsCap = idsCap = 0;
        }
        ~PinnedBuffers() { Dispose(); }
    }

    /// <summary>The result of GpuTikTokenizer.EncodeBatchFlatPinned: the ids of all texts in page-locked memory, text t at [Offsets[t], Offsets[t + 1]).
    /// Owns a buffer set of the tokenizer's pool until it is disposed.</summary>
    public sealed class FlatBatchResult : IDisposable
    {
        private readonly GpuTikTokenizer owner; private PinnedBuffers holder;
        public long[] Offsets { get; }
        public long Count => Offsets[Offsets.Length - 1];
        public IntPtr Ids => holder != null ? holder.Ids(0) : throw new ObjectDisposedException(nameof(FlatBatchResult));
        internal FlatBatchResult(GpuTikTokenizer owner, PinnedBuffers holder, long[] offsets) { this.owner = owner; this.holder = holder; Offsets = offsets; }
        public unsafe int this[long i] => ((int*)Ids)[i];
        /// <summary>The ids of text t as a managed array.</summary>
        public unsafe int[] Text(int t)
        {
            long n = Offsets[t + 1] - Offsets[t];
            var a = new int[n];
            if (n > 0) fixed (int* dst = a) Buffer.MemoryCopy((int*)Ids + Offsets[t], dst, n * 4, n * 4);
            return a;
        }
        public void Dispose() { PinnedBuffers h = System.Threading.Interlocked.Exchange(ref holder, null); if (h != null) owner.ReturnBuffers(h); }
    }

    public sealed class GpuTikTokenizer : ITokenizer, IDisposable
    {
        private readonly EncoderHandle handle;
        private IntPtr encoder => handle.DangerousGetHandle();
        private readonly IReadOnlyDictionary<string, int> specialTokensEncoder;
        private readonly HashSet<string> specialTokens;         // Contains() only: the alternation below keeps the dictionary's order
        private readonly Regex specialTokensRegex;

        /// <summary>Same arguments as TokenizerBuilder.CreateTokenizer (TokenizerBuilder.cs:210-213) plus the HIP device index.</summary>
        /// <param name="reserveBytes">when &gt; 0: the device workspace of batches of up to this many UTF-8 bytes (in up to reserveDocs texts) is allocated here,
        /// by the constructor, instead of inside the first EncodeBatch (tkz_encoder_reserve: ~7.8 device bytes per byte of text)</param>
        public GpuTikTokenizer(Stream tikTokenBpeFileStream, IReadOnlyDictionary<string, int> specialTokensEncoder, string pattern, int cacheSize = 8192, int device = 0,
                               long reserveBytes = 0, long reserveDocs = 0)
        {
            byte[] file;
            using (var ms = new MemoryStream()) { tikTokenBpeFileStream.CopyTo(ms); file = ms.ToArray(); }
            Tkz.Check(Tkz.tkz_pattern_from_regex(Tkz.Utf8Z(pattern), out int pat));   // only the reference's own three patterns are implemented
            Tkz.Check(Tkz.tkz_vocab_from_tiktoken(file, (UIntPtr)file.Length, out IntPtr vocab));
            IntPtr enc;
            try { Tkz.Check(Tkz.tkz_encoder_create(vocab, pat, device, out enc)); }
            finally { Tkz.tkz_vocab_destroy(vocab); }
            handle = new EncoderHandle(enc);
            this.specialTokensEncoder = specialTokensEncoder;
            specialTokens = new HashSet<string>(specialTokensEncoder.Keys);
            // the alternation in the order of specialTokensEncoder.Keys, as the reference builds it (TikTokenizer.cs:78): when one
            // special token is a prefix of another, the order of the alternatives decides the match
            specialTokensRegex = new Regex(string.Join("|", specialTokensEncoder.Keys.Select(s => Regex.Escape(s))), RegexOptions.Compiled);
            RegisterSpecialTokensForDecode();
            // the LRU piece memo (LRUCache.cs; no effect on results) lives on the device with a fixed size: cacheSize says whether it is used
            if (cacheSize <= 0) Tkz.Check(Tkz.tkz_encoder_set_option(handle.DangerousGetHandle(), 2 /* TKZ_OPT_PIECE_MEMO */, 0));
            UseThisRuntimesRegexSemantics();
            if (reserveBytes > 0) Tkz.Check(Tkz.tkz_encoder_reserve(encoder, reserveBytes, Math.Max(1, reserveDocs)));
        }

        /// <summary>The reference's split is `new Regex(pattern, RegexOptions.Compiled)` of the RUNNING process (TikTokenizer.cs:77): \p{L}, \p{N} ... are the
        /// categories of this runtime's Unicode data (13.0 under net6.0, 15.0 under .NET 8) and (?i:...) is this runtime's case folding (ASCII pairs up to
        /// .NET 6; the case-equivalence tables from .NET 7 on, under which U+017F is an `s`).  libtkz is built for net6.0; here it is told what THIS
        /// runtime says: the class of every UTF-16 code unit (all that pattern 1, cl100k and the o200k string through .NET's engine ever look at), and
        /// the case mode.</summary>
        private void UseThisRuntimesRegexSemantics()
        {
            var classes = new byte[65536];
            for (int c = 0; c < 65536; ++c)
            {
                char ch = (char)c;
                byte k;
                switch (char.GetUnicodeCategory(ch))
                {
                    case System.Globalization.UnicodeCategory.UppercaseLetter: k = 1; break;
                    case System.Globalization.UnicodeCategory.LowercaseLetter: k = 2; break;
                    case System.Globalization.UnicodeCategory.TitlecaseLetter: k = 3; break;
                    case System.Globalization.UnicodeCategory.ModifierLetter: k = 4; break;
                    case System.Globalization.UnicodeCategory.OtherLetter: k = 5; break;
                    case System.Globalization.UnicodeCategory.NonSpacingMark:
                    case System.Globalization.UnicodeCategory.SpacingCombiningMark:
                    case System.Globalization.UnicodeCategory.EnclosingMark: k = 6; break;
                    case System.Globalization.UnicodeCategory.DecimalDigitNumber:
                    case System.Globalization.UnicodeCategory.LetterNumber:
                    case System.Globalization.UnicodeCategory.OtherNumber: k = 7; break;
                    // \s of System.Text.RegularExpressions: [\f\n\r\t\v\x85\p{Z}]
                    case System.Globalization.UnicodeCategory.SpaceSeparator:
                    case System.Globalization.UnicodeCategory.LineSeparator:
                    case System.Globalization.UnicodeCategory.ParagraphSeparator: k = 8; break;
                    default: k = (byte)((c >= 9 && c <= 13) || c == 0x85 ? 8 : 0); break;
                }
                classes[c] = k;
            }
            Tkz.Check(Tkz.tkz_encoder_set_unicode_classes(encoder, classes, classes.Length));
            // Environment.Version: 4.x on .NET Framework, 3.1 on .NET Core 3.1, 5 / 6 / 7 / 8 ... on .NET 5+
            Tkz.Check(Tkz.tkz_encoder_set_option(encoder, 7 /* TKZ_OPT_CASE_EQUIVALENCE */, Environment.Version.Major >= 7 ? 1 : 0));
        }

        // SpecialTokensDecoder (TikTokenizer.cs:79) for the device Decode
        private unsafe void RegisterSpecialTokensForDecode()
        {
            if (specialTokensEncoder.Count == 0) return;
            var ids = specialTokensEncoder.Values.ToArray();
            var lits = specialTokensEncoder.Keys.Select(k => Encoding.UTF8.GetBytes(k)).ToArray();
            var offs = new long[lits.Length + 1];
            for (int i = 0; i < lits.Length; ++i) offs[i + 1] = offs[i] + lits[i].Length;
            var blob = new byte[Math.Max(1, offs[lits.Length])];
            for (int i = 0; i < lits.Length; ++i) lits[i].CopyTo(blob, offs[i]);
            fixed (int* pi = ids) fixed (byte* pb = blob) fixed (long* po = offs)
                Tkz.Check(Tkz.tkz_encoder_set_special_tokens(encoder, pi, pb, po, ids.Length));
        }

        public List<int> Encode(string text, IReadOnlyCollection<string> allowedSpecial)
            => SpecialOnDevice(text, allowedSpecial) ?? EncodeBatch(new[] { text }, allowedSpecial)[0];

        public List<int> Encode(string text, bool applySpecialTokens = true)
            => Encode(text, applySpecialTokens && specialTokens.Count > 0 ? (IReadOnlyCollection<string>)specialTokens : Array.Empty<string>());

        // Encode(text, allowedSpecial) on one string: ONE call of tkz_encode_special_utf16 on the string's own chars -- one kernel launch for a prompt.  null: nothing
        // to allow (the plain route of EncodeBatch), or the registered set is beyond the device path (-7): the host segmentation of EncodeBatchFlat from now on.
        private unsafe List<int>? SpecialOnDevice(string text, IReadOnlyCollection<string>? allowedSpecial)
        {
            if (allowedSpecial is null || allowedSpecial.Count == 0 || specialTokensEncoder.Count == 0 || specialOnHost) return null;
            var index = new List<int>();                                              // registration order = the alternation's
            { int i = 0; foreach (string k in specialTokensEncoder.Keys) { if (allowedSpecial.Contains(k)) index.Add(i); ++i; } }
            int[] allowed = index.Count > 0 ? index.ToArray() : new int[1];
            long cap = Math.Max(1, Math.Min(3L * text.Length, text.Length / 2 + 4096));   // (a token per two units first; 3 * units always suffice)
            while (true)
            {
                var ids = new int[cap];
                int st; long n;
                fixed (char* pc = text) fixed (int* pa = allowed) fixed (int* pi = ids)
                    st = Tkz.tkz_encode_special_utf16(encoder, pc, text.Length, index.Count > 0 ? pa : null, index.Count, pi, cap, out n);
                if (st == -7) { specialOnHost = true; return null; }
                if (st == -4 /* TKZ_E_CAPACITY */ && n > cap) { cap = n; continue; }
                Tkz.Check(st);
                GC.KeepAlive(this);
                var result = new List<int>((int)n);
                if (n > 0) result.AddRange(new ArraySegment<int>(ids, 0, (int)n));
                return result;
            }
        }

        /// <summary>Encode(text, allowedSpecial).Count without the ids: ONE call of tkz_count_utf16 on the string's own chars (a single kernel launch for a prompt,
        /// nothing but the count comes back).  With a registered set the device path does not hold (-7) it is Encode(...).Count.</summary>
        public unsafe int CountTokens(string text, IReadOnlyCollection<string> allowedSpecial)
        {
            bool plain = allowedSpecial is null || allowedSpecial.Count == 0 || specialTokensEncoder.Count == 0;
            if (plain || !specialOnHost)
            {
                int[] allowed = plain ? Array.Empty<int>() : AllowedIndex(allowedSpecial!);
                int st; long n;
                fixed (char* pc = text) fixed (int* pa = allowed)
                    st = Tkz.tkz_count_utf16(encoder, pc, text.Length, allowed.Length > 0 ? pa : null, allowed.Length, out n);
                GC.KeepAlive(this);
                if (st != -7) { Tkz.Check(st); return checked((int)n); }
                specialOnHost = true;
            }
            return Encode(text, allowedSpecial!).Count;
        }

        public int CountTokens(string text, bool applySpecialTokens = true)
            => CountTokens(text, applySpecialTokens && specialTokens.Count > 0 ? (IReadOnlyCollection<string>)specialTokens : Array.Empty<string>());

        /// <summary>The count of every text, as CountTokens(text, allowedSpecial) gives it: the strings' chars go to tkz_count_batch_utf16 as they are (copied into one
        /// char[] with string.CopyTo), only the offsets come back.</summary>
        public unsafe int[] CountTokensBatch(IReadOnlyList<string> texts, IReadOnlyCollection<string>? allowedSpecial = null)
        {
            var counts = new int[texts.Count];
            if (texts.Count == 0) return counts;
            bool plain = allowedSpecial is null || allowedSpecial.Count == 0 || specialTokensEncoder.Count == 0;
            if (plain || !specialOnHost)
            {
                var unitOffsets = new long[texts.Count + 1];
                for (int t = 0; t < texts.Count; ++t) unitOffsets[t + 1] = unitOffsets[t] + texts[t].Length;
                var units = new char[Math.Max(1, unitOffsets[texts.Count])];
                for (int t = 0; t < texts.Count; ++t) texts[t].CopyTo(0, units, (int)unitOffsets[t], texts[t].Length);
                int[] allowed = plain ? Array.Empty<int>() : AllowedIndex(allowedSpecial!);
                var offsets = new long[texts.Count + 1];
                int st;
                fixed (char* pu = units) fixed (long* po = unitOffsets) fixed (int* pa = allowed) fixed (long* pt = offsets)
                    st = Tkz.tkz_count_batch_utf16(encoder, pu, po, texts.Count, allowed.Length > 0 ? pa : null, allowed.Length, pt, out _);
                GC.KeepAlive(this);
                if (st != -7)
                {
                    Tkz.Check(st);
                    for (int t = 0; t < texts.Count; ++t) counts[t] = checked((int)(offsets[t + 1] - offsets[t]));
                    return counts;
                }
                specialOnHost = true;
            }
            var lists = EncodeBatch(texts, allowedSpecial);
            for (int t = 0; t < texts.Count; ++t) counts[t] = lists[t].Count;
            return counts;
        }

        /// <summary>Encode(text, allowedSpecial) and, per token, the index in <paramref name="text"/> (chars, i.e. UTF-16 code units) where the token's text starts --
        /// EncodeToTokens' Offset.  Token t is text[starts[t] .. starts[t + 1]), the last one ends at text.Length.  A token that starts inside a character (byte-level
        /// BPE splits emoji and CJK under an English vocabulary) starts AFTER that character's chars, and a token of continuation bytes only has an empty span.
        /// ONE call of tkz_encode_batch_spans_utf16.  A registered set the device path does not hold is NotImplementedException (-7): there is no host path.</summary>
        public (List<int> Ids, List<int> Starts) EncodeWithOffsets(string text, IReadOnlyCollection<string>? allowedSpecial = null)
        {
            var (ids, starts) = EncodeWithOffsetsBatch(new[] { text }, allowedSpecial);
            return (ids[0], starts[0]);
        }

        /// <summary>EncodeWithOffsets for every text: the strings' chars go to tkz_encode_batch_spans_utf16 as they are (copied into one char[] with string.CopyTo).</summary>
        public unsafe (List<List<int>> Ids, List<List<int>> Starts) EncodeWithOffsetsBatch(IReadOnlyList<string> texts, IReadOnlyCollection<string>? allowedSpecial = null)
        {
            var outIds = new List<List<int>>(texts.Count);
            var outStarts = new List<List<int>>(texts.Count);
            if (texts.Count == 0) return (outIds, outStarts);
            bool plain = allowedSpecial is null || allowedSpecial.Count == 0 || specialTokensEncoder.Count == 0;
            var unitOffsets = new long[texts.Count + 1];
            for (int t = 0; t < texts.Count; ++t) unitOffsets[t + 1] = unitOffsets[t] + texts[t].Length;
            var units = new char[Math.Max(1, unitOffsets[texts.Count])];
            for (int t = 0; t < texts.Count; ++t) texts[t].CopyTo(0, units, (int)unitOffsets[t], texts[t].Length);
            int[] allowed = plain ? Array.Empty<int>() : AllowedIndex(allowedSpecial!);
            long cap = Math.Max(1, 3 * unitOffsets[texts.Count]);              // a token per byte, a char is at most three bytes
            var ids = new int[cap];
            var starts = new int[cap];
            var offsets = new long[texts.Count + 1];
            int st;
            fixed (char* pu = units) fixed (long* po = unitOffsets) fixed (int* pa = allowed) fixed (int* pi = ids) fixed (int* ps = starts) fixed (long* pt = offsets)
                st = Tkz.tkz_encode_batch_spans_utf16(encoder, pu, po, texts.Count, allowed.Length > 0 ? pa : null, allowed.Length, pi, cap, pt, ps, out _);
            GC.KeepAlive(this);
            Tkz.Check(st);
            for (int t = 0; t < texts.Count; ++t)
            {
                int lo = checked((int)offsets[t]), n = checked((int)(offsets[t + 1] - offsets[t]));
                var li = new List<int>(n); li.AddRange(new ArraySegment<int>(ids, lo, n));
                var ls = new List<int>(n); ls.AddRange(new ArraySegment<int>(starts, lo, n));
                outIds.Add(li); outStarts.Add(ls);
            }
            return (outIds, outStarts);
        }

        /// <summary>The text cut into chunks of at most <paramref name="maxTokenCount"/> tokens, in ONE call: what a loop over EncodeTrimSuffix on the rest of the
        /// string yields while no piece exceeds the budget -- and, where that loop would never end (the next piece alone holds more tokens), runs of maxTokenCount
        /// tokens of that piece, the last partial run going on with the pieces that follow (include/tkz.h states the rule).  The ids concatenate to Encode's, the
        /// texts to the input; a character cut by a chunk boundary goes to the earlier chunk.  maxTokenCount below 1 is ArgumentOutOfRangeException.  A registered set
        /// the device path does not hold is NotImplementedException (-7): there is no host path.</summary>
        public List<(List<int> TokenIds, string Text)> EncodeChunks(string text, IReadOnlyCollection<string>? allowedSpecial, int maxTokenCount)
        {
            return EncodeChunksBatch(new[] { text }, allowedSpecial, maxTokenCount)[0];
        }

        /// <summary>EncodeChunks for every text: the strings' chars go to tkz_encode_batch_chunks_utf16 as they are (copied into one char[] with string.CopyTo).</summary>
        public unsafe List<List<(List<int> TokenIds, string Text)>> EncodeChunksBatch(IReadOnlyList<string> texts, IReadOnlyCollection<string>? allowedSpecial, int maxTokenCount)
        {
            if (maxTokenCount < 1) throw new ArgumentOutOfRangeException(nameof(maxTokenCount));
            var result = new List<List<(List<int> TokenIds, string Text)>>(texts.Count);
            if (texts.Count == 0) return result;
            bool plain = allowedSpecial is null || allowedSpecial.Count == 0 || specialTokensEncoder.Count == 0;
            var unitOffsets = new long[texts.Count + 1];
            for (int t = 0; t < texts.Count; ++t) unitOffsets[t + 1] = unitOffsets[t] + texts[t].Length;
            long total = unitOffsets[texts.Count];
            var units = new char[Math.Max(1, total)];
            for (int t = 0; t < texts.Count; ++t) texts[t].CopyTo(0, units, (int)unitOffsets[t], texts[t].Length);
            int[] allowed = plain ? Array.Empty<int>() : AllowedIndex(allowedSpecial!);
            long cap = Math.Max(1, 3 * total);                                   // a token per byte, a char is at most three bytes
            long chunkCap = Math.Max(1, Math.Min(3 * total, texts.Count + 2 * (3 * total) / maxTokenCount));      // the chunks that always suffice (tkz.h)
            var ids = new int[cap];
            var offsets = new long[texts.Count + 1];
            var docChunks = new long[texts.Count + 1];
            var chunkTokens = new long[chunkCap + 1];
            var chunkUnits = new long[chunkCap];
            int st;
            fixed (char* pu = units) fixed (long* po = unitOffsets) fixed (int* pa = allowed) fixed (int* pi = ids) fixed (long* pt = offsets) fixed (long* pd = docChunks)
            fixed (long* pc = chunkTokens) fixed (long* pn = chunkUnits)
                st = Tkz.tkz_encode_batch_chunks_utf16(encoder, pu, po, texts.Count, allowed.Length > 0 ? pa : null, allowed.Length, maxTokenCount, pi, cap, pt, pd, pc, pn, chunkCap,
                                                       out _, out _);
            GC.KeepAlive(this);
            Tkz.Check(st);
            for (int t = 0; t < texts.Count; ++t)
            {
                var chunks = new List<(List<int> TokenIds, string Text)>(checked((int)(docChunks[t + 1] - docChunks[t])));
                for (long c = docChunks[t]; c < docChunks[t + 1]; ++c)
                {
                    int lo = checked((int)chunkTokens[c]), n = checked((int)(chunkTokens[c + 1] - chunkTokens[c]));
                    var li = new List<int>(n); li.AddRange(new ArraySegment<int>(ids, lo, n));
                    int a = checked((int)chunkUnits[c]), b = c + 1 < docChunks[t + 1] ? checked((int)chunkUnits[c + 1]) : texts[t].Length;
                    chunks.Add((li, texts[t].Substring(a, b - a)));
                }
                result.Add(chunks);
            }
            return result;
        }

        /// <summary>EncodeChunks with an overlap, as text splitters take it: consecutive chunks share at most <paramref name="overlap"/> tokens and the text of
        /// those tokens.  A chunk is what EncodeTrimSuffix(rest, maxTokenCount) returns; the next one starts with what EncodeTrimPrefix(chunk text, overlap) keeps --
        /// one item further on when that is the whole chunk, behind the chunk when a chunk begun there would end where this one does (include/tkz.h states the
        /// rule).  overlap 0 gives EncodeChunks' result.  maxTokenCount below 1 and an overlap outside [0, maxTokenCount) are ArgumentOutOfRangeException.  A
        /// registered set the device path does not hold is NotImplementedException (-7): there is no host path.</summary>
        public List<(List<int> TokenIds, string Text)> EncodeChunksOverlap(string text, IReadOnlyCollection<string>? allowedSpecial, int maxTokenCount, int overlap)
        {
            return EncodeChunksOverlapBatch(new[] { text }, allowedSpecial, maxTokenCount, overlap)[0];
        }

        /// <summary>EncodeChunksOverlap for every text, in ONE call of tkz_encode_batch_chunks_overlap_utf16: every chunk is the ids [start, end) and the chars
        /// [start unit, end unit) of its text.</summary>
        public unsafe List<List<(List<int> TokenIds, string Text)>> EncodeChunksOverlapBatch(IReadOnlyList<string> texts, IReadOnlyCollection<string>? allowedSpecial,
                                                                                              int maxTokenCount, int overlap)
        {
            if (maxTokenCount < 1) throw new ArgumentOutOfRangeException(nameof(maxTokenCount));
            if (overlap < 0 || overlap >= maxTokenCount) throw new ArgumentOutOfRangeException(nameof(overlap));
            var result = new List<List<(List<int> TokenIds, string Text)>>(texts.Count);
            if (texts.Count == 0) return result;
            bool plain = allowedSpecial is null || allowedSpecial.Count == 0 || specialTokensEncoder.Count == 0;
            var unitOffsets = new long[texts.Count + 1];
            for (int t = 0; t < texts.Count; ++t) unitOffsets[t + 1] = unitOffsets[t] + texts[t].Length;
            long total = unitOffsets[texts.Count];
            var units = new char[Math.Max(1, total)];
            for (int t = 0; t < texts.Count; ++t) texts[t].CopyTo(0, units, (int)unitOffsets[t], texts[t].Length);
            int[] allowed = plain ? Array.Empty<int>() : AllowedIndex(allowedSpecial!);
            long cap = Math.Max(1, 3 * total);                                   // a token per byte, a char is at most three bytes
            long chunkCap = Math.Max(1, Math.Min(3 * total, texts.Count + 2 * (3 * total) / (maxTokenCount - overlap)));      // the chunks that always suffice (tkz.h)
            var ids = new int[cap];
            var offsets = new long[texts.Count + 1];
            var docChunks = new long[texts.Count + 1];
            var chunkTokens = new long[chunkCap];
            var chunkEnds = new long[chunkCap];
            var chunkUnits = new long[chunkCap];
            var chunkEndUnits = new long[chunkCap];
            int st;
            fixed (char* pu = units) fixed (long* po = unitOffsets) fixed (int* pa = allowed) fixed (int* pi = ids) fixed (long* pt = offsets) fixed (long* pd = docChunks)
            fixed (long* pc = chunkTokens) fixed (long* pe = chunkEnds) fixed (long* pn = chunkUnits) fixed (long* pm = chunkEndUnits)
                st = Tkz.tkz_encode_batch_chunks_overlap_utf16(encoder, pu, po, texts.Count, allowed.Length > 0 ? pa : null, allowed.Length, maxTokenCount, overlap, pi, cap, pt, pd,
                                                               pc, pe, pn, pm, chunkCap, out _, out _);
            GC.KeepAlive(this);
            Tkz.Check(st);
            for (int t = 0; t < texts.Count; ++t)
            {
                var chunks = new List<(List<int> TokenIds, string Text)>(checked((int)(docChunks[t + 1] - docChunks[t])));
                for (long c = docChunks[t]; c < docChunks[t + 1]; ++c)
                {
                    int lo = checked((int)chunkTokens[c]), n = checked((int)(chunkEnds[c] - chunkTokens[c]));
                    var li = new List<int>(n); li.AddRange(new ArraySegment<int>(ids, lo, n));
                    int a = checked((int)chunkUnits[c]), b = checked((int)chunkEndUnits[c]);
                    chunks.Add((li, texts[t].Substring(a, b - a)));
                }
                result.Add(chunks);
            }
            return result;
        }

        /// <summary>Every text's ids -- Encode's for the same arguments -- with <paramref name="bos"/> in front and <paramref name="eos"/> behind it (null: none;
        /// any id of 0 or more is taken as it is), the stream cut into rows of <paramref name="rowLen"/> and padded with <paramref name="pad"/>, in ONE call
        /// (tkz_encode_batch_packed_utf16; include/tkz.h states the rule).  Ids and Pos are rows x rowLen; Pos restarts at every text and every row; SegStarts
        /// (cu_seqlens) ends with the stream's length; DocOffsets[d] is where text d starts in the stream.  A registered set the device path does not hold is
        /// NotImplementedException (-7): there is no host path.</summary>
        public unsafe (int[,] Ids, int[,] Pos, long[] SegStarts, long[] DocOffsets) EncodeBatchPacked(IReadOnlyList<string> texts, int rowLen,
                                                                                                      IReadOnlyCollection<string>? allowedSpecial = null, int? bos = null,
                                                                                                      int? eos = null, int pad = 0)
        {
            if (rowLen < 1) throw new ArgumentOutOfRangeException(nameof(rowLen));
            if (bos < 0 || eos < 0) throw new ArgumentOutOfRangeException(bos < 0 ? nameof(bos) : nameof(eos));
            bool plain = allowedSpecial is null || allowedSpecial.Count == 0 || specialTokensEncoder.Count == 0;
            var unitOffsets = new long[texts.Count + 1];
            for (int t = 0; t < texts.Count; ++t) unitOffsets[t + 1] = unitOffsets[t] + texts[t].Length;
            long total = unitOffsets[texts.Count];
            var units = new char[Math.Max(1, total)];
            for (int t = 0; t < texts.Count; ++t) texts[t].CopyTo(0, units, (int)unitOffsets[t], texts[t].Length);
            int[] allowed = plain ? Array.Empty<int>() : AllowedIndex(allowedSpecial!);
            int framing = (bos.HasValue ? 1 : 0) + (eos.HasValue ? 1 : 0);
            long rowsBound = (3 * total + (long)framing * texts.Count + rowLen - 1) / rowLen;      // the sizes that always suffice (tkz.h): a token per byte, a char is at most three bytes
            long cap = rowsBound * rowLen, segCap = texts.Count + rowsBound;
            var ids = new int[Math.Max(1, cap)];
            var pos = new int[Math.Max(1, cap)];
            var seg = new long[segCap + 1];
            var offsets = new long[texts.Count + 1];
            int st;
            long neededIds, neededSegs;
            fixed (char* pu = units) fixed (long* po = unitOffsets) fixed (int* pa = allowed) fixed (int* pi = ids) fixed (int* pp = pos) fixed (long* ps = seg) fixed (long* pt = offsets)
                st = Tkz.tkz_encode_batch_packed_utf16(encoder, pu, po, texts.Count, allowed.Length > 0 ? pa : null, allowed.Length, bos ?? -1, eos ?? -1, rowLen, pad, pi, cap, pt,
                                                       pp, ps, segCap, out _, out neededIds, out neededSegs);
            GC.KeepAlive(this);
            Tkz.Check(st);
            int rows = checked((int)(neededIds / rowLen));
            var outIds = new int[rows, rowLen];
            var outPos = new int[rows, rowLen];
            Buffer.BlockCopy(ids, 0, outIds, 0, checked((int)(neededIds * sizeof(int))));
            Buffer.BlockCopy(pos, 0, outPos, 0, checked((int)(neededIds * sizeof(int))));
            var segStarts = new long[neededSegs + 1];
            Array.Copy(seg, segStarts, neededSegs + 1);
            return (outIds, outPos, segStarts, offsets);
        }

        /// <summary>Every text's ids -- Encode's for the same arguments -- cut to <paramref name="maxLength"/> less the framing (<paramref name="truncateLeft"/>: the tail
        /// is kept, else the head), with <paramref name="bos"/> in front and <paramref name="eos"/> behind what is kept (null: none; any id of 0 or more is taken as it
        /// is), a row a text, padded with <paramref name="pad"/> (on the left with <paramref name="padLeft"/>) to the longest row rounded up to
        /// <paramref name="padToMultipleOf"/> -- at most maxLength; 0: to maxLength itself --, in ONE call (tkz_encode_batch_padded_utf16; include/tkz.h states the rule).
        /// Ids, Mask (1 on content) and Pos (the index inside the content) are texts x width; Lens the content lengths.  The cut is a plain cut of the id list, not
        /// EncodeTrimSuffix's whole-item cut.  A registered set the device path does not hold is NotImplementedException (-7): there is no host path.</summary>
        public unsafe (int[,] Ids, byte[,] Mask, int[,] Pos, int[] Lens) EncodeBatchPadded(IReadOnlyList<string> texts, int maxLength, IReadOnlyCollection<string>? allowedSpecial = null,
                                                                                          int? bos = null, int? eos = null, int pad = 0, bool truncateLeft = false, bool padLeft = false,
                                                                                          int padToMultipleOf = 1)
        {
            int framing = (bos.HasValue ? 1 : 0) + (eos.HasValue ? 1 : 0);
            if (maxLength < Math.Max(1, framing)) throw new ArgumentOutOfRangeException(nameof(maxLength));
            if (bos < 0 || eos < 0) throw new ArgumentOutOfRangeException(bos < 0 ? nameof(bos) : nameof(eos));
            if (padToMultipleOf < 0) throw new ArgumentOutOfRangeException(nameof(padToMultipleOf));
            bool plain = allowedSpecial is null || allowedSpecial.Count == 0 || specialTokensEncoder.Count == 0;
            var unitOffsets = new long[texts.Count + 1];
            for (int t = 0; t < texts.Count; ++t) unitOffsets[t + 1] = unitOffsets[t] + texts[t].Length;
            long total = unitOffsets[texts.Count];
            var units = new char[Math.Max(1, total)];
            for (int t = 0; t < texts.Count; ++t) texts[t].CopyTo(0, units, (int)unitOffsets[t], texts[t].Length);
            int[] allowed = plain ? Array.Empty<int>() : AllowedIndex(allowedSpecial!);
            long cap = (long)texts.Count * maxLength;                                            // the size that always suffices (tkz.h): a row of maxLength a text
            var ids = new int[Math.Max(1, cap)];
            var pos = new int[Math.Max(1, cap)];
            var mask = new byte[Math.Max(1, cap)];
            var lens = new int[Math.Max(1, texts.Count)];
            int st;
            long width;
            fixed (char* pu = units) fixed (long* po = unitOffsets) fixed (int* pa = allowed) fixed (int* pi = ids) fixed (int* pp = pos) fixed (byte* pm = mask) fixed (int* pl = lens)
                st = Tkz.tkz_encode_batch_padded_utf16(encoder, pu, po, texts.Count, allowed.Length > 0 ? pa : null, allowed.Length, bos ?? -1, eos ?? -1, maxLength,
                                                       truncateLeft ? 1 : 0, padLeft ? 1 : 0, pad, padToMultipleOf, pi, cap, pm, pp, pl, null, out _, out width, out _);
            GC.KeepAlive(this);
            Tkz.Check(st);
            int w = checked((int)width);
            var outIds = new int[texts.Count, w];
            var outPos = new int[texts.Count, w];
            var outMask = new byte[texts.Count, w];
            Buffer.BlockCopy(ids, 0, outIds, 0, checked(texts.Count * w * sizeof(int)));
            Buffer.BlockCopy(pos, 0, outPos, 0, checked(texts.Count * w * sizeof(int)));
            Buffer.BlockCopy(mask, 0, outMask, 0, checked(texts.Count * w));
            var outLens = new int[texts.Count];
            Array.Copy(lens, outLens, texts.Count);
            return (outIds, outMask, outPos, outLens);
        }

        /// <summary>EncodeBatchPadded's rows with the texts sorted by content length (<paramref name="descending"/>: longest first; equal lengths keep the texts' order),
        /// cut into buckets of <paramref name="bucketRows"/> sorted rows, every bucket padded to ITS OWN longest row (rounded up to <paramref name="padToMultipleOf"/>, at
        /// most maxLength; 0: to maxLength itself), in ONE call (tkz_encode_batch_bucketed_utf16; include/tkz.h states the rule).  Buckets[b] holds Ids and Mask of
        /// rows x width; its row i is text Order[b * bucketRows + i]; Rank is the inverse of Order; Lens are in the texts' order.</summary>
        public unsafe ((int[,] Ids, byte[,] Mask)[] Buckets, long[] Order, long[] Rank, int[] Lens) EncodeBatchBucketed(IReadOnlyList<string> texts, int maxLength, int bucketRows,
                                                                                                                       IReadOnlyCollection<string>? allowedSpecial = null, int? bos = null,
                                                                                                                       int? eos = null, int pad = 0, bool descending = false,
                                                                                                                       bool truncateLeft = false, bool padLeft = false, int padToMultipleOf = 1)
        {
            int framing = (bos.HasValue ? 1 : 0) + (eos.HasValue ? 1 : 0);
            if (maxLength < Math.Max(1, framing)) throw new ArgumentOutOfRangeException(nameof(maxLength));
            if (bucketRows < 1) throw new ArgumentOutOfRangeException(nameof(bucketRows));
            if (bos < 0 || eos < 0) throw new ArgumentOutOfRangeException(bos < 0 ? nameof(bos) : nameof(eos));
            if (padToMultipleOf < 0) throw new ArgumentOutOfRangeException(nameof(padToMultipleOf));
            bool plain = allowedSpecial is null || allowedSpecial.Count == 0 || specialTokensEncoder.Count == 0;
            var unitOffsets = new long[texts.Count + 1];
            for (int t = 0; t < texts.Count; ++t) unitOffsets[t + 1] = unitOffsets[t] + texts[t].Length;
            long total = unitOffsets[texts.Count];
            var units = new char[Math.Max(1, total)];
            for (int t = 0; t < texts.Count; ++t) texts[t].CopyTo(0, units, (int)unitOffsets[t], texts[t].Length);
            int[] allowed = plain ? Array.Empty<int>() : AllowedIndex(allowedSpecial!);
            long cap = (long)texts.Count * maxLength;                                            // the size that always suffices (tkz.h): a row of maxLength a text
            int nBuckets = (texts.Count + bucketRows - 1) / bucketRows;
            var ids = new int[Math.Max(1, cap)];
            var mask = new byte[Math.Max(1, cap)];
            var lens = new int[Math.Max(1, texts.Count)];
            var order = new long[Math.Max(1, texts.Count)];
            var rank = new long[Math.Max(1, texts.Count)];
            var bucketOffsets = new long[nBuckets + 1];
            var bucketWidths = new int[Math.Max(1, nBuckets)];
            int st;
            fixed (char* pu = units) fixed (long* po = unitOffsets) fixed (int* pa = allowed) fixed (int* pi = ids) fixed (byte* pm = mask) fixed (int* pl = lens)
            fixed (long* pr = order) fixed (long* pk = rank) fixed (long* pb = bucketOffsets) fixed (int* pw = bucketWidths)
                st = Tkz.tkz_encode_batch_bucketed_utf16(encoder, pu, po, texts.Count, allowed.Length > 0 ? pa : null, allowed.Length, bos ?? -1, eos ?? -1, maxLength,
                                                         truncateLeft ? 1 : 0, padLeft ? 1 : 0, pad, padToMultipleOf, bucketRows, descending ? 1 : 0, pi, cap, pm, null, pl, null,
                                                         pr, pk, pb, pw, out _, out _, out _);
            GC.KeepAlive(this);
            Tkz.Check(st);
            var buckets = new (int[,] Ids, byte[,] Mask)[nBuckets];
            for (int b = 0; b < nBuckets; ++b)
            {
                int rows = Math.Min(bucketRows, texts.Count - b * bucketRows), w = bucketWidths[b];
                var bIds = new int[rows, w];
                var bMask = new byte[rows, w];
                Buffer.BlockCopy(ids, checked((int)bucketOffsets[b] * sizeof(int)), bIds, 0, checked(rows * w * sizeof(int)));
                Buffer.BlockCopy(mask, checked((int)bucketOffsets[b]), bMask, 0, checked(rows * w));
                buckets[b] = (bIds, bMask);
            }
            var outLens = new int[texts.Count];
            var outOrder = new long[texts.Count];
            var outRank = new long[texts.Count];
            Array.Copy(lens, outLens, texts.Count);
            Array.Copy(order, outOrder, texts.Count);
            Array.Copy(rank, outRank, texts.Count);
            return (buckets, outOrder, outRank, outLens);
        }

        /// <summary>EncodeBatchBucketed's sorted rows cut greedily by a TOKEN budget: a bucket takes rows while rows x width is at most <paramref name="maxTokens"/>
        /// (the width of its longest row, rounded up to <paramref name="padToMultipleOf"/>, at most maxLength; 0: maxLength itself) and it has at most
        /// <paramref name="maxRows"/> rows (null: no cap), in ONE call (tkz_encode_batch_budgeted_utf16; include/tkz.h states the rule).  Buckets[b] holds Ids and Mask
        /// of rows x width; the rows of the buckets, one after the other, are the texts Order[0], Order[1], ...; Rank is the inverse of Order; Lens are in the texts'
        /// order.  (Written out beside EncodeBatchBucketed; like it, not compiled where this repository is built.)</summary>
        public unsafe ((int[,] Ids, byte[,] Mask)[] Buckets, long[] Order, long[] Rank, int[] Lens) EncodeBatchBudgeted(IReadOnlyList<string> texts, int maxLength, long maxTokens,
                                                                                                                       int? maxRows = null,
                                                                                                                       IReadOnlyCollection<string>? allowedSpecial = null, int? bos = null,
                                                                                                                       int? eos = null, int pad = 0, bool descending = false,
                                                                                                                       bool truncateLeft = false, bool padLeft = false, int padToMultipleOf = 1)
        {
            int framing = (bos.HasValue ? 1 : 0) + (eos.HasValue ? 1 : 0);
            if (maxLength < Math.Max(1, framing)) throw new ArgumentOutOfRangeException(nameof(maxLength));
            if (maxTokens < maxLength || maxTokens > 1L << 62) throw new ArgumentOutOfRangeException(nameof(maxTokens));
            if (maxRows < 1) throw new ArgumentOutOfRangeException(nameof(maxRows));
            if (bos < 0 || eos < 0) throw new ArgumentOutOfRangeException(bos < 0 ? nameof(bos) : nameof(eos));
            if (padToMultipleOf < 0) throw new ArgumentOutOfRangeException(nameof(padToMultipleOf));
            bool plain = allowedSpecial is null || allowedSpecial.Count == 0 || specialTokensEncoder.Count == 0;
            var unitOffsets = new long[texts.Count + 1];
            for (int t = 0; t < texts.Count; ++t) unitOffsets[t + 1] = unitOffsets[t] + texts[t].Length;
            long total = unitOffsets[texts.Count];
            var units = new char[Math.Max(1, total)];
            for (int t = 0; t < texts.Count; ++t) texts[t].CopyTo(0, units, (int)unitOffsets[t], texts[t].Length);
            int[] allowed = plain ? Array.Empty<int>() : AllowedIndex(allowedSpecial!);
            long cap = (long)texts.Count * maxLength;                                            // the sizes that always suffice (tkz.h): a row of maxLength and a bucket a text
            var ids = new int[Math.Max(1, cap)];
            var mask = new byte[Math.Max(1, cap)];
            var lens = new int[Math.Max(1, texts.Count)];
            var order = new long[Math.Max(1, texts.Count)];
            var rank = new long[Math.Max(1, texts.Count)];
            var bucketOffsets = new long[texts.Count + 1];
            var bucketRows = new long[texts.Count + 1];
            var bucketWidths = new int[Math.Max(1, texts.Count)];
            int st;
            long nBuckets;
            fixed (char* pu = units) fixed (long* po = unitOffsets) fixed (int* pa = allowed) fixed (int* pi = ids) fixed (byte* pm = mask) fixed (int* pl = lens)
            fixed (long* pr = order) fixed (long* pk = rank) fixed (long* pb = bucketOffsets) fixed (long* ps = bucketRows) fixed (int* pw = bucketWidths)
                st = Tkz.tkz_encode_batch_budgeted_utf16(encoder, pu, po, texts.Count, allowed.Length > 0 ? pa : null, allowed.Length, bos ?? -1, eos ?? -1, maxLength,
                                                         truncateLeft ? 1 : 0, padLeft ? 1 : 0, pad, padToMultipleOf, maxTokens, maxRows ?? int.MaxValue, descending ? 1 : 0, pi, cap,
                                                         pm, null, pl, null, pr, pk, pb, ps, pw, texts.Count, out _, out _, out _, out nBuckets);
            GC.KeepAlive(this);
            Tkz.Check(st);
            var buckets = new (int[,] Ids, byte[,] Mask)[nBuckets];
            for (int b = 0; b < nBuckets; ++b)
            {
                int rows = checked((int)(bucketRows[b + 1] - bucketRows[b])), w = bucketWidths[b];
                var bIds = new int[rows, w];
                var bMask = new byte[rows, w];
                Buffer.BlockCopy(ids, checked((int)bucketOffsets[b] * sizeof(int)), bIds, 0, checked(rows * w * sizeof(int)));
                Buffer.BlockCopy(mask, checked((int)bucketOffsets[b]), bMask, 0, checked(rows * w));
                buckets[b] = (bIds, bMask);
            }
            var outLens = new int[texts.Count];
            var outOrder = new long[texts.Count];
            var outRank = new long[texts.Count];
            Array.Copy(lens, outLens, texts.Count);
            Array.Copy(order, outOrder, texts.Count);
            Array.Copy(rank, outRank, texts.Count);
            return (buckets, outOrder, outRank, outLens);
        }

        /// <summary>How a pair of texts is cut to the maximum length (tkz_pair_truncation, include/tkz.h): an id at a time from the longer text -- from the second on
        /// a tie --, the first text only (the second once nothing of the first is left), or the second text only.</summary>
        public enum PairTruncation { LongestFirst = 0, OnlyFirst = 1, OnlySecond = 2 }

        /// <summary>Row i holds <paramref name="first"/>[i] and <paramref name="second"/>[i] as a cross-encoder takes them: <paramref name="bos"/>, the first text's ids,
        /// <paramref name="sepCount"/> (0..2) times <paramref name="sep"/>, the second text's ids, <paramref name="eos"/> (null: none; any id of 0 or more is taken as it
        /// is) -- Encode's ids for the same arguments, the two lists cut to <paramref name="maxLength"/> less the framing TOGETHER by <paramref name="truncation"/>
        /// (<paramref name="truncateLeft"/>: the tails are kept, else the heads), padded with <paramref name="pad"/> (on the left with <paramref name="padLeft"/>) to the
        /// longest row rounded up to <paramref name="padToMultipleOf"/> -- at most maxLength; 0: to maxLength itself --, in ONE call (tkz_encode_batch_pairs_utf16;
        /// include/tkz.h states the rule).  Ids, Mask (1 on content) and TypeIds (1 on the second text's ids and the eos) are pairs x width; Lens the content lengths;
        /// Kept the ids kept of either text.  A registered set the device path does not hold is NotImplementedException (-7): there is no host path.</summary>
        public unsafe (int[,] Ids, byte[,] Mask, byte[,] TypeIds, int[] Lens, int[,] Kept) EncodeBatchPairs(IReadOnlyList<string> first, IReadOnlyList<string> second, int maxLength,
                                                                                                             IReadOnlyCollection<string>? allowedSpecial = null, int? bos = null,
                                                                                                             int? sep = null, int sepCount = 1, int? eos = null, int pad = 0,
                                                                                                             PairTruncation truncation = PairTruncation.LongestFirst,
                                                                                                             bool truncateLeft = false, bool padLeft = false, int padToMultipleOf = 1)
        {
            if (first.Count != second.Count) throw new ArgumentException("first and second must hold as many texts as each other", nameof(second));
            if (sepCount < 0 || sepCount > 2) throw new ArgumentOutOfRangeException(nameof(sepCount));
            if (!sep.HasValue) sepCount = 0;
            int framing = (bos.HasValue ? 1 : 0) + sepCount + (eos.HasValue ? 1 : 0);
            if (maxLength < Math.Max(1, framing)) throw new ArgumentOutOfRangeException(nameof(maxLength));
            if (bos < 0 || sep < 0 || eos < 0) throw new ArgumentOutOfRangeException(bos < 0 ? nameof(bos) : sep < 0 ? nameof(sep) : nameof(eos));
            if (padToMultipleOf < 0) throw new ArgumentOutOfRangeException(nameof(padToMultipleOf));
            bool plain = allowedSpecial is null || allowedSpecial.Count == 0 || specialTokensEncoder.Count == 0;
            int pairs = first.Count, docs = 2 * pairs;
            var unitOffsets = new long[docs + 1];                                                 // documents 2p and 2p + 1: the two texts of pair p
            for (int p = 0; p < pairs; ++p)
            {
                unitOffsets[2 * p + 1] = unitOffsets[2 * p] + first[p].Length;
                unitOffsets[2 * p + 2] = unitOffsets[2 * p + 1] + second[p].Length;
            }
            long total = unitOffsets[docs];
            var units = new char[Math.Max(1, total)];
            for (int p = 0; p < pairs; ++p)
            {
                first[p].CopyTo(0, units, (int)unitOffsets[2 * p], first[p].Length);
                second[p].CopyTo(0, units, (int)unitOffsets[2 * p + 1], second[p].Length);
            }
            int[] allowed = plain ? Array.Empty<int>() : AllowedIndex(allowedSpecial!);
            long cap = (long)pairs * maxLength;                                                   // the size that always suffices (tkz.h): a row of maxLength a pair
            var ids = new int[Math.Max(1, cap)];
            var mask = new byte[Math.Max(1, cap)];
            var types = new byte[Math.Max(1, cap)];
            var lens = new int[Math.Max(1, pairs)];
            var kept = new int[Math.Max(1, docs)];
            int st;
            long width;
            fixed (char* pu = units) fixed (long* po = unitOffsets) fixed (int* pa = allowed) fixed (int* pi = ids) fixed (byte* pm = mask) fixed (byte* pt = types) fixed (int* pl = lens)
            fixed (int* pk = kept)
                st = Tkz.tkz_encode_batch_pairs_utf16(encoder, pu, po, docs, allowed.Length > 0 ? pa : null, allowed.Length, bos ?? -1, sep ?? -1, sepCount, eos ?? -1, maxLength,
                                                      (int)truncation, truncateLeft ? 1 : 0, padLeft ? 1 : 0, pad, padToMultipleOf, pi, cap, pm, pt, null, pl, pk, null,
                                                      out _, out width, out _);
            GC.KeepAlive(this);
            Tkz.Check(st);
            int w = checked((int)width);
            var outIds = new int[pairs, w];
            var outMask = new byte[pairs, w];
            var outTypes = new byte[pairs, w];
            Buffer.BlockCopy(ids, 0, outIds, 0, checked(pairs * w * sizeof(int)));
            Buffer.BlockCopy(mask, 0, outMask, 0, checked(pairs * w));
            Buffer.BlockCopy(types, 0, outTypes, 0, checked(pairs * w));
            var outLens = new int[pairs];
            Array.Copy(lens, outLens, pairs);
            var outKept = new int[pairs, 2];
            Buffer.BlockCopy(kept, 0, outKept, 0, checked(docs * sizeof(int)));
            return (outIds, outMask, outTypes, outLens, outKept);
        }

        // the allowed literals as indices into the registered set (registration order = the alternation's)
        private int[] AllowedIndex(IReadOnlyCollection<string> allowedSpecial)
        {
            var index = new List<int>();
            int i = 0;
            foreach (string k in specialTokensEncoder.Keys) { if (allowedSpecial.Contains(k)) index.Add(i); ++i; }
            return index.ToArray();
        }

        /// <summary>Encodes every text as Encode(text, allowedSpecial) would; all plain segments go to the GPU as one batch.
        /// One List per text, each filled with ONE AddRange over its segment of the flat result.</summary>
        public List<List<int>> EncodeBatch(IReadOnlyList<string> texts, IReadOnlyCollection<string>? allowedSpecial = null)
        {
            var (ids, offsets) = EncodeBatchFlat(texts, allowedSpecial);
            var result = new List<List<int>>(texts.Count);
            for (int t = 0; t < texts.Count; ++t)
            {
                int n = (int)(offsets[t + 1] - offsets[t]);
                var one = new List<int>(n);
                if (n > 0) one.AddRange(new ArraySegment<int>(ids, (int)offsets[t], n));      // (ICollection<int>.CopyTo: one block copy)
                result.Add(one);
            }
            return result;
        }

        /// <summary>EncodeBatch without a List per text: text t is Ids[Offsets[t] .. Offsets[t + 1]).  When no special token applies
        /// (the reference's plain path, TikTokenizer.cs:180-183,196-199) Offsets is the device call's own output and Ids holds exactly
        /// Offsets[texts.Count] ids; otherwise the special ids are spliced in between the plain segments' ids with block copies.</summary>
        public unsafe (int[] Ids, long[] Offsets) EncodeBatchFlat(IReadOnlyList<string> texts, IReadOnlyCollection<string>? allowedSpecial = null)
        {
            bool plain = allowedSpecial is null || allowedSpecial.Count == 0 || specialTokensEncoder.Count == 0;
            // 0. special tokens: the whole texts to the device's UTF-16 special entry, which cuts the allowed literals out itself.  Only a registered set the device
            //    path does not hold (TKZ_E_UNSUPPORTED, -7) is segmented here, from then on.
            if (!plain && !specialOnHost)
            {
                var onDevice = SpecialBatchOnDevice(texts, allowedSpecial!);
                if (onDevice.HasValue) return onDevice.Value;
            }
            // 1. segmentation on the host: (text index, plain segment) and literal special ids, in order
            var plan = new List<(int text, int special, int segment)>();
            var segments = new List<(string text, int start, int end)>(texts.Count);
            for (int t = 0; t < texts.Count; ++t)
            {
                string text = texts[t];
                if (plain)
                {
                    segments.Add((text, 0, text.Length));                     // (one segment per text, empty ones included: the offsets line up)
                    continue;
                }
                int start = 0;
                while (text.Length > 0)
                {
                    Match next; int startFind = start;
                    while (true)                                              // FindNextSpecialToken (TikTokenizer.cs:230-241)
                    {
                        next = specialTokensRegex.Match(text, startFind);
                        if (!next.Success || allowedSpecial!.Contains(next.Value)) break;
                        startFind = next.Index + 1;
                    }
                    int end = next.Success ? next.Index : text.Length;
                    if (end > start) { plan.Add((t, -1, segments.Count)); segments.Add((text, start, end)); }
                    if (!next.Success) break;
                    plan.Add((t, specialTokensEncoder[next.Value], -1));        // EncodeSpecialToken (:215-220)
                    start = next.Index + next.Length;
                    if (start >= text.Length) break;
                }
            }
            // 2. the plain segments through the device (EncodeSegments below: page-locked buffers, sub-batches, the gather ahead of the device call); the ids
            //    arrive in ONE page-locked buffer and leave it as a managed array of exactly their number -- `new int[]` is zero-filled by the runtime and
            //    then written: on a million texts that copy is the larger part of this method's time, which is why EncodeBatchFlatPinned exists
            var segOffsets = new long[segments.Count + 1];
            int[] ids;
            PinnedBuffers holder = EncodeSegments(segments, segOffsets);
            try
            {
                long n = segOffsets[segments.Count];
                ids = new int[Math.Max(1, n)];
                IntPtr src = holder.Ids(0);
                int parts = (int)Math.Max(1, Math.Min(Environment.ProcessorCount, n >> 20));     // (first touch of a fresh array: page faults, spread over the cores)
                System.Threading.Tasks.Parallel.For(0, parts, part =>
                {
                    long lo = n * part / parts, hi = n * (part + 1) / parts;
                    fixed (int* dst = ids) Buffer.MemoryCopy((int*)src + lo, dst + lo, (hi - lo) * 4, (hi - lo) * 4);
                });
            }
            finally { ReturnBuffers(holder); }
            if (plain) return (ids, segOffsets);
            // 3. splice the special ids in: block copies of the segments' id ranges
            long nSpecial = 0;
            foreach (var item in plan) if (item.segment < 0) ++nSpecial;
            var flat = new int[Math.Max(1, segOffsets[segments.Count] + nSpecial)];
            var offsets = new long[texts.Count + 1];
            long w = 0; int cur = 0;
            foreach (var (t, special, segment) in plan)
            {
                while (cur < t) offsets[++cur] = w;
                if (segment < 0) { flat[w++] = special; continue; }
                long n = segOffsets[segment + 1] - segOffsets[segment];
                Array.Copy(ids, segOffsets[segment], flat, w, n);
                w += n;
            }
            while (cur < texts.Count) offsets[++cur] = w;
            return (flat, offsets);
        }

        private const long SubBatchUnits = 64L << 20;                          // code units per device call of a large batch (128 MB)
        private readonly System.Collections.Concurrent.ConcurrentBag<PinnedBuffers> bufferPool = new System.Collections.Concurrent.ConcurrentBag<PinnedBuffers>();
        private volatile bool disposed;
        private long tokensPerUnitQ20;                                           // the densest batch seen, tokens per code unit << 20: sizes the id buffer of the next one
        private PinnedBuffers RentBuffers()
        {
            if (disposed) throw new ObjectDisposedException(nameof(GpuTikTokenizer));
            return bufferPool.TryTake(out PinnedBuffers b) ? b : new PinnedBuffers();
        }
        internal void ReturnBuffers(PinnedBuffers b)
        {
            if (disposed) { b.Dispose(); GC.SuppressFinalize(b); } else bufferPool.Add(b);
        }

        /// <summary>The plain segments as batches of UTF-16 code units in PAGE-LOCKED memory (tkz_host_alloc; buffer sets are pooled, one per call in flight:
        /// concurrent EncodeBatch callers do not wait for one another -- the library leases a workspace per call as well).  The strings are copied by all
        /// cores (Parallel.For over slices); Encoding.UTF8.GetBytes (TikTokenizer.cs:261) is done for the whole batch on the device by
        /// tkz_encode_batch_utf16.  A large batch goes in SUB-BATCHES of ~128 MB of code units: the gather of sub-batch k + 1 runs while the device encodes
        /// sub-batch k (two unit buffers), as include/tkz_tokenizer.hpp's EncodeBatchFlat does.  Every sub-batch's ids are written by the device call straight
        /// behind those of the one before, into ONE page-locked buffer: the returned set's Ids(0), segOffsets[segments.Count] of them; segOffsets are global.
        /// The caller gives the returned set back with ReturnBuffers.</summary>
        private unsafe PinnedBuffers EncodeSegments(List<(string text, int start, int end)> segments, long[] segOffsets)
        {
            int nseg = segments.Count;
            var unitOffsets = new long[nseg + 1];
            long total = 0;
            for (int i = 0; i < nseg; ++i) { unitOffsets[i] = total; total += segments[i].end - segments[i].start; }
            unitOffsets[nseg] = total;
            var cuts = new List<int> { 0 };                                   // sub-batch k = segments [cuts[k], cuts[k + 1])
            for (int i = 1; i < nseg; ++i)
                if (unitOffsets[i + 1] - unitOffsets[cuts[cuts.Count - 1]] > SubBatchUnits) cuts.Add(i);
            cuts.Add(nseg);
            int nsub = cuts.Count - 1;
            // A code unit is at most three UTF-8 bytes and a token at least one byte, so 3 * total ids always suffice; English text has a token per ~4 units
            // and CJK text about one per unit: the buffer gets room for what the densest batch so far needed (+ 10 %), a token per two units at least, and
            // grows -- keeping what is in it -- when a sub-batch reports TKZ_E_CAPACITY (-4): once in a tokenizer's life per kind of text, not once per batch.
            long learnt = (long)((double)total * (System.Threading.Interlocked.Read(ref tokensPerUnitQ20) / 1048576.0) * 1.1);
            long cap = Math.Max(1, Math.Min(3 * total, Math.Max(total / 2 + 4096, learnt)));
            PinnedBuffers holder = RentBuffers();                             // its Units: sub-batches 0, 2, 4 ...; its Ids: the whole batch's
            PinnedBuffers second = nsub > 1 ? RentBuffers() : null;           // its Units: sub-batches 1, 3, 5 ...
            bool ok = false;
            try
            {
                holder.Ids(cap * 4);
                long[] state = { 0, cap };                                    // ids so far; capacity of the id buffer (both only touched by the one device call in flight)
                System.Threading.Tasks.Task pending = null;
                for (int k = 0; k < nsub; ++k)
                {
                    PinnedBuffers set = (k & 1) == 0 ? holder : second;       // (its Units were last read by sub-batch k - 2, whose call has been waited for)
                    int lo = cuts[k], hi = cuts[k + 1], n = hi - lo;
                    long u0 = unitOffsets[lo], nu = unitOffsets[hi] - u0;
                    IntPtr unitsPtr = set.Units((nu + 32) * 2);               // (an IntPtr: a lambda cannot capture a pointer-typed local)
                    int slices = Math.Max(1, Math.Min(Environment.ProcessorCount, n / 4096));
                    System.Threading.Tasks.Parallel.For(0, slices, sl =>
                    {
                        char* dstUnits = (char*)unitsPtr;
                        int a = lo + (int)((long)n * sl / slices), b = lo + (int)((long)n * (sl + 1) / slices);
                        for (int i = a; i < b; ++i)
                        {
                            int len = segments[i].end - segments[i].start;
                            if (len == 0) continue;
                            fixed (char* src = segments[i].text)
                                Buffer.MemoryCopy(src + segments[i].start, dstUnits + (unitOffsets[i] - u0), (long)len * 2, (long)len * 2);
                        }
                    });
                    if (pending != null) pending.Wait();                      // the device call of sub-batch k - 1 (its exception surfaces here)
                    pending = System.Threading.Tasks.Task.Run(() => EncodeSubBatch(holder, unitsPtr, unitOffsets, lo, n, nu, total - u0, segOffsets, state));
                }
                if (pending != null) pending.Wait();
                if (total > 0)
                {
                    long q = (long)((double)state[0] / total * 1048576.0), seen;
                    while ((seen = System.Threading.Interlocked.Read(ref tokensPerUnitQ20)) < q &&
                           System.Threading.Interlocked.CompareExchange(ref tokensPerUnitQ20, q, seen) != seen) { }
                }
                ok = true;
                return holder;
            }
            finally
            {
                if (second != null) ReturnBuffers(second);
                if (!ok) ReturnBuffers(holder);
            }
        }
        // One device call: the n segments from `lo` on, nu code units at unitsPtr, their ids behind the state[0] ids already in holder's id buffer
        // (capacity state[1]); fills segOffsets[lo + 1 .. lo + n] (global) and advances state[0].  unitsLeft: code units from this sub-batch to the batch's end.
        private unsafe void EncodeSubBatch(PinnedBuffers holder, IntPtr unitsPtr, long[] unitOffsets, int lo, int n, long nu, long unitsLeft, long[] segOffsets, long[] state)
        {
            var rel = new long[n + 1];
            long u0 = unitOffsets[lo];
            for (int i = 0; i <= n; ++i) rel[i] = unitOffsets[lo + i] - u0;
            var outOffs = new long[n + 1];
            long needed;
            bool held = false;
            try
            {
                handle.DangerousAddRef(ref held);                                // (Dispose on another thread: the native encoder outlives this call)
                while (true)
                {
                    long done = state[0], room = state[1] - done;
                    int* pi = (int*)holder.Ids(0) + done;
                    int st;
                    fixed (long* po = rel) fixed (long* poo = outOffs)
                        st = Tkz.tkz_encode_batch_utf16(encoder, (char*)unitsPtr, po, n, pi, room, poo, out needed);
                    if (st == -4 && needed > room)
                    {   // this sub-batch needs `needed`; what follows it, at the same density at least
                        long want = done + needed + (long)((double)needed / Math.Max(1, nu) * (unitsLeft - nu) * 1.1) + 4096;
                        holder.GrowIdsKeeping(done * 4, want * 4);
                        state[1] = want;
                        continue;
                    }
                    Tkz.Check(st);
                    break;
                }
            }
            finally { if (held) handle.DangerousRelease(); }
            for (int i = 1; i <= n; ++i) segOffsets[lo + i] = state[0] + outOffs[i];
            state[0] += needed;
            GC.KeepAlive(holder);                                                // (the buffers' finalizer must not run while the native call reads them)
            GC.KeepAlive(this);
        }

        /// <summary>EncodeBatchFlat with the ids LEFT in page-locked memory (no special tokens: the reference's plain path, TikTokenizer.cs:180-183): text t is
        /// ids [Offsets[t], Offsets[t + 1]) of the result.  Nothing is copied after the device has written the ids -- on a million texts the managed
        /// `int[]` of EncodeBatchFlat (zero-filled by the runtime, then written) costs more than the encoding.  Dispose the result to give the buffers back.</summary>
        public FlatBatchResult EncodeBatchFlatPinned(IReadOnlyList<string> texts)
        {
            var segments = new List<(string text, int start, int end)>(texts.Count);
            for (int t = 0; t < texts.Count; ++t) segments.Add((texts[t], 0, texts[t].Length));
            var offsets = new long[texts.Count + 1];
            PinnedBuffers holder = EncodeSegments(segments, offsets);
            return new FlatBatchResult(this, holder, offsets);
        }

        // One item per regex piece of every plain segment and one per special token, in order: its ids and its length in
        // UTF-16 units (piece.Length / nextSpecial.Value.Length of TikTokenizer.cs:295,367).
        private unsafe List<(int[] Ids, int Length)> PieceItems(string text, IReadOnlyCollection<string>? allowedSpecial)
        {
            var plan = new List<(int special, int start, int end)>();          // special < 0: plain segment text[start..end]
            int start = 0;
            while (text.Length > 0)
            {
                Match? next = null; int end = text.Length;
                if (allowedSpecial != null && allowedSpecial.Count > 0)
                {
                    int startFind = start;
                    while (true)                                              // FindNextSpecialToken (TikTokenizer.cs:230-241)
                    {
                        next = specialTokensRegex.Match(text, startFind);
                        if (!next.Success || allowedSpecial.Contains(next.Value)) break;
                        startFind = next.Index + 1;
                    }
                    if (next.Success) end = next.Index;
                }
                if (end > start) plan.Add((-1, start, end));
                if (next is null || !next.Success) break;
                plan.Add((specialTokensEncoder[next.Value], next.Index, next.Index + next.Length));
                start = next.Index + next.Length;
                if (start >= text.Length) break;
            }
            var segs = plan.Where(p => p.special < 0).ToList();
            var offsets = new long[segs.Count + 1];
            long total = 0;
            fixed (char* pc = text)                                          // (the char* overloads: netstandard2.0 has no Span)
                for (int i = 0; i < segs.Count; ++i) { offsets[i] = total; total += Encoding.UTF8.GetByteCount(pc + segs[i].start, segs[i].end - segs[i].start); }
            offsets[segs.Count] = total;
            var bytes = new byte[Math.Max(1, total)];
            fixed (char* pc = text) fixed (byte* pbytes = bytes)
                for (int i = 0; i < segs.Count; ++i)
                    Encoding.UTF8.GetBytes(pc + segs[i].start, segs[i].end - segs[i].start, pbytes + offsets[i], (int)(offsets[i + 1] - offsets[i]));
            int cap = (int)Math.Max(1, total);
            var ids = new int[cap]; var dpo = new long[segs.Count + 1]; var pbo = new long[cap + 1]; var pto = new long[cap + 1];
            fixed (byte* pb = bytes) fixed (long* po = offsets) fixed (int* pi = ids) fixed (long* pd = dpo) fixed (long* pp = pbo) fixed (long* pt = pto)
                Tkz.Check(Tkz.tkz_encode_batch_pieces_utf8(encoder, pb, po, segs.Count, pi, cap, pd, pp, pt, cap, out _, out _));
            var items = new List<(int[] Ids, int Length)>();
            int k = 0;
            foreach (var (special, s0, e0) in plan)
            {
                if (special >= 0) { items.Add((new[] { special }, e0 - s0)); continue; }
                for (long p = dpo[k]; p < dpo[k + 1]; ++p)
                {
                    var tok = new int[pto[p + 1] - pto[p]];
                    Array.Copy(ids, pto[p], tok, 0, tok.Length);
                    // UTF-16 length of the piece: chars + supplementary-plane chars (lead bytes, 0xF0.. counted twice)
                    int len = 0;
                    for (long b = pbo[p]; b < pbo[p + 1]; ++b) { if ((bytes[b] & 0xC0) != 0x80) ++len; if (bytes[b] >= 0xF0) ++len; }
                    items.Add((tok, len));
                }
                ++k;
            }
            return items;
        }

        // the texts' chars in one array (string.CopyTo: no GetBytes on the host), their offsets in code units, the indices of the allowed literals
        private (char[] Units, long[] Offsets, int[] Allowed, int NAllowed) GatherUnits(IReadOnlyList<string> texts, IReadOnlyCollection<string>? allowedSpecial, bool plain)
        {
            var index = new List<int>();                                              // registration order = the alternation's
            if (!plain) { int i = 0; foreach (string k in specialTokensEncoder.Keys) { if (allowedSpecial!.Contains(k)) index.Add(i); ++i; } }
            var offsets = new long[texts.Count + 1];
            for (int t = 0; t < texts.Count; ++t) offsets[t + 1] = offsets[t] + texts[t].Length;
            var units = new char[Math.Max(1, offsets[texts.Count])];
            for (int t = 0; t < texts.Count; ++t) texts[t].CopyTo(0, units, (int)offsets[t], texts[t].Length);
            return (units, offsets, index.Count > 0 ? index.ToArray() : new int[1], index.Count);
        }

        // Encode(text, allowedSpecial) for a batch: ONE call of tkz_encode_batch_special_utf16 on the strings' own chars.  null: the registered set is beyond the
        // device path (-7), the host segmentation of EncodeBatchFlat does it from now on.
        private unsafe (int[] Ids, long[] Offsets)? SpecialBatchOnDevice(IReadOnlyList<string> texts, IReadOnlyCollection<string> allowedSpecial)
        {
            var (units, offsets, allowed, nAllowed) = GatherUnits(texts, allowedSpecial, false);
            var outOffs = new long[texts.Count + 1];
            long total = offsets[texts.Count], cap = Math.Max(1, Math.Min(3 * total, total / 2 + 4096));     // (a token per two units first; 3 * units always suffice)
            while (true)
            {
                var ids = new int[cap];
                int st; long needed;
                fixed (char* pc = units) fixed (long* po = offsets) fixed (int* pa = allowed) fixed (int* pi = ids) fixed (long* poo = outOffs)
                    st = Tkz.tkz_encode_batch_special_utf16(encoder, pc, po, texts.Count, nAllowed > 0 ? pa : null, nAllowed, pi, cap, poo, out needed);
                if (st == -7) { specialOnHost = true; return null; }
                if (st == -4 /* TKZ_E_CAPACITY */ && needed > cap) { cap = needed; continue; }
                Tkz.Check(st);
                GC.KeepAlive(this);
                return (ids, outOffs);
            }
        }

        // EncodeTrimSuffix / EncodeTrimPrefix for a batch of texts: ONE device call (tkz_encode_batch_trim_utf16 on the strings' own chars -- transcoded, the literals
        // cut out, the pieces counted, the cut chosen and the kept ids compacted on the device; cutUnits is the reference's encodeLength / actualPrefixStrLength).
        // Returns null when the host walk over PieceItems has to do it: a registered set the device path does not hold (TKZ_E_UNSUPPORTED, -7), a negative maximum.
        // (A lone surrogate under a literal that holds U+FFFD needs no host route any more: the device knows which U+FFFD it wrote itself.)
        private bool specialOnHost;
        private unsafe List<(List<int> TokenIds, string Text)>? TrimBatchOnDevice(IReadOnlyList<string> texts, IReadOnlyCollection<string>? allowedSpecial, int maxTokenCount, int side)
        {
            bool plain = allowedSpecial is null || allowedSpecial.Count == 0 || specialTokensEncoder.Count == 0;
            if (maxTokenCount < 0 || (!plain && specialOnHost)) return null;
            var result = new List<(List<int> TokenIds, string Text)>(texts.Count);
            if (texts.Count == 0) return result;
            var (units, offsets, allowed, nAllowed) = GatherUnits(texts, allowedSpecial, plain);
            long total = offsets[texts.Count];
            long cap = Math.Min(3 * total, (long)texts.Count * maxTokenCount);        // (tkz.h: always sufficient)
            var ids = new int[Math.Max(1, cap)]; var outOffs = new long[texts.Count + 1]; var cutUnits = new long[texts.Count];
            int st;
            fixed (char* pc = units) fixed (long* po = offsets) fixed (int* pa = allowed) fixed (int* pi = ids) fixed (long* poo = outOffs) fixed (long* pu = cutUnits)
                st = Tkz.tkz_encode_batch_trim_utf16(encoder, pc, po, texts.Count, nAllowed > 0 ? pa : null, nAllowed, side, maxTokenCount, null, pi, cap, poo, pu, out _);
            if (st == -7) { specialOnHost = true; return null; }
            Tkz.Check(st);
            for (int t = 0; t < texts.Count; ++t)
            {
                var kept = new List<int>((int)(outOffs[t + 1] - outOffs[t]));
                for (long k = outOffs[t]; k < outOffs[t + 1]; ++k) kept.Add(ids[k]);
                int u = (int)cutUnits[t];
                result.Add((kept, side == 0 ? (u == texts[t].Length ? texts[t] : texts[t].Substring(0, u)) : (u == 0 ? texts[t] : texts[t].Substring(u))));
            }
            GC.KeepAlive(this);
            return result;
        }

        // ONE text: ONE call of tkz_encode_trim_utf16 on the string's own chars -- one kernel launch for a prompt.  null: the host walk has to do it, in the
        // cases of TrimBatchOnDevice.  (Like the rest of this file: not compiled here.)
        private unsafe (List<int> TokenIds, string Text)? TrimOneOnDevice(string text, IReadOnlyCollection<string>? allowedSpecial, int maxTokenCount, int side)
        {
            bool plain = allowedSpecial is null || allowedSpecial.Count == 0 || specialTokensEncoder.Count == 0;
            if (maxTokenCount < 0 || (!plain && specialOnHost)) return null;
            var index = new List<int>();                                              // registration order = the alternation's
            if (!plain) { int i = 0; foreach (string k in specialTokensEncoder.Keys) { if (allowedSpecial!.Contains(k)) index.Add(i); ++i; } }
            int[] allowed = index.Count > 0 ? index.ToArray() : new int[1];
            long cap = Math.Min(3L * text.Length, maxTokenCount);                     // (the KEPT ids: tkz.h)
            var ids = new int[Math.Max(1, cap)];
            int st; long n, cutUnits;
            fixed (char* pc = text) fixed (int* pa = allowed) fixed (int* pi = ids)
                st = Tkz.tkz_encode_trim_utf16(encoder, pc, text.Length, index.Count > 0 ? pa : null, index.Count, side, maxTokenCount, pi, cap, out n, out cutUnits);
            if (st == -7) { specialOnHost = true; return null; }
            Tkz.Check(st);
            GC.KeepAlive(this);
            var kept = new List<int>((int)n);
            if (n > 0) kept.AddRange(new ArraySegment<int>(ids, 0, (int)n));
            int u = (int)cutUnits;
            return (kept, side == 0 ? (u == text.Length ? text : text.Substring(0, u)) : (u == 0 ? text : text.Substring(u)));
        }

        public List<(List<int> TokenIds, string Text)> EncodeTrimSuffixBatch(IReadOnlyList<string> texts, IReadOnlyCollection<string> allowedSpecial, int maxTokenCount)
            => TrimBatchOnDevice(texts, allowedSpecial, maxTokenCount, 0 /* TKZ_TRIM_SUFFIX */) ?? texts.Select(t => TrimSuffixOnHost(t, allowedSpecial, maxTokenCount)).ToList();
        public List<(List<int> TokenIds, string Text)> EncodeTrimSuffixBatch(IReadOnlyList<string> texts, int maxTokenCount, bool applySpecialTokens = true)
            => EncodeTrimSuffixBatch(texts, applySpecialTokens && specialTokens.Count > 0 ? specialTokens : null!, maxTokenCount);
        public List<(List<int> TokenIds, string Text)> EncodeTrimPrefixBatch(IReadOnlyList<string> texts, IReadOnlyCollection<string> allowedSpecial, int maxTokenCount)
            => TrimBatchOnDevice(texts, allowedSpecial, maxTokenCount, 1 /* TKZ_TRIM_PREFIX */) ?? texts.Select(t => TrimPrefixOnHost(t, allowedSpecial, maxTokenCount)).ToList();
        public List<(List<int> TokenIds, string Text)> EncodeTrimPrefixBatch(IReadOnlyList<string> texts, int maxTokenCount, bool applySpecialTokens = true)
            => EncodeTrimPrefixBatch(texts, applySpecialTokens && specialTokens.Count > 0 ? specialTokens : null!, maxTokenCount);

        public (List<int> TokenIds, string Text) EncodeTrimSuffix(string text, IReadOnlyCollection<string> allowedSpecial, int maxTokenCount)
            => TrimOneOnDevice(text, allowedSpecial, maxTokenCount, 0 /* TKZ_TRIM_SUFFIX */) ?? TrimSuffixOnHost(text, allowedSpecial, maxTokenCount);
        // the host walk over the pieces: the fallback of the batch methods
        private (List<int> TokenIds, string Text) TrimSuffixOnHost(string text, IReadOnlyCollection<string> allowedSpecial, int maxTokenCount)
        {
            var tokenIds = new List<int>();
            int tokenCount = 0, encodeLength = 0;
            foreach (var (ids, length) in PieceItems(text, allowedSpecial))           // the walk of TikTokenizer.cs:288-341 / :343-392
            {
                tokenCount += ids.Length;
                if (tokenCount > maxTokenCount) break;                            // the piece that overflows is dropped, with everything after it
                tokenIds.AddRange(ids);
                encodeLength += length;
                if (tokenCount >= maxTokenCount) break;
            }
            return (tokenIds, encodeLength == text.Length ? text : text.Substring(0, encodeLength));
        }
        public (List<int> TokenIds, string Text) EncodeTrimSuffix(string text, int maxTokenCount, bool applySpecialTokens = true)
            => EncodeTrimSuffix(text, applySpecialTokens && specialTokens.Count > 0 ? specialTokens : null!, maxTokenCount);

        public (List<int> TokenIds, string Text) EncodeTrimPrefix(string text, IReadOnlyCollection<string> allowedSpecial, int maxTokenCount)
            => TrimOneOnDevice(text, allowedSpecial, maxTokenCount, 1 /* TKZ_TRIM_PREFIX */) ?? TrimPrefixOnHost(text, allowedSpecial, maxTokenCount);
        private (List<int> TokenIds, string Text) TrimPrefixOnHost(string text, IReadOnlyCollection<string> allowedSpecial, int maxTokenCount)
        {
            var tokenIds = new List<int>();
            int tokenCount = 0, encodeLength = 0;
            var tokenCountMap = new SortedDictionary<int, int> { { 0, 0 } };          // TikTokenizer.cs:438-441
            foreach (var (ids, length) in PieceItems(text, allowedSpecial))
            {
                tokenCount += ids.Length; encodeLength += length;
                tokenIds.AddRange(ids);
                tokenCountMap[tokenCount] = encodeLength;
            }
            if (tokenCount <= maxTokenCount) return (tokenIds, text);                  // TrimPrefix (:470-483)
            int prefixTokenCount = tokenCount - maxTokenCount, cutTokens = 0, cutLength = 0;
            foreach (var pair in tokenCountMap) if (pair.Key >= prefixTokenCount) { cutTokens = pair.Key; cutLength = pair.Value; break; }
            return (tokenIds.GetRange(cutTokens, tokenIds.Count - cutTokens), text.Substring(cutLength));
        }
        public (List<int> TokenIds, string Text) EncodeTrimPrefix(string text, int maxTokenCount, bool applySpecialTokens = true)
            => EncodeTrimPrefix(text, applySpecialTokens && specialTokens.Count > 0 ? specialTokens : null!, maxTokenCount);

        /// <summary>TikTokenizer.Decode (TikTokenizer.cs:586-604): ids in neither table are dropped; on the device, Encoding.UTF8.GetString (:603)
        /// included -- tkz_decode_batch_utf16 hands back the code units of every document, one U+FFFD per maximal subpart of an ill-formed sequence as
        /// GetString writes them, and each string is built from its unit range.  The strings are those GetString gives on the bytes of tkz_decode_batch.
        /// ONE id list goes through tkz_decode_utf16 -- a single kernel launch for up to 32,768 ids -- into a pooled buffer (a ConcurrentBag of char[], as the
        /// page-locked sets are pooled: netstandard2.0 has no ArrayPool without a package).  A buffer that was too small is dropped, the larger one is kept.</summary>
        private readonly System.Collections.Concurrent.ConcurrentBag<char[]> decodePool = new System.Collections.Concurrent.ConcurrentBag<char[]>();
        public unsafe string Decode(int[] tokens)
        {
            if (tokens.Length == 0) return string.Empty;
            int want = Math.Max(256, 8 * tokens.Length);
            if (!decodePool.TryTake(out char[] units) || units.Length < want) units = new char[want];
            try
            {
                while (true)
                {
                    int st; long n;
                    fixed (int* pi = tokens) fixed (char* pu = units)
                        st = Tkz.tkz_decode_utf16(encoder, pi, tokens.Length, pu, units.Length, out n);
                    if (st == -4) { units = new char[checked((int)n)]; continue; }     // TKZ_E_CAPACITY: `n` is the exact size, in code units
                    Tkz.Check(st);
                    return new string(units, 0, (int)n);
                }
            }
            finally { if (!disposed) decodePool.Add(units); }
        }

        public unsafe List<string> DecodeBatch(IReadOnlyList<int[]> batches)
        {
            var offs = new long[batches.Count + 1];
            for (int i = 0; i < batches.Count; ++i) offs[i + 1] = offs[i] + batches[i].Length;
            var flat = new int[Math.Max(1, offs[batches.Count])];
            for (int i = 0; i < batches.Count; ++i) batches[i].CopyTo(flat, offs[i]);
            var outOffs = new long[batches.Count + 1];
            var units = new char[Math.Max(16, 8 * flat.Length)];
            while (true)
            {
                int st; long needed;
                fixed (int* pi = flat) fixed (long* po = offs) fixed (char* pu = units) fixed (long* poo = outOffs)
                    st = Tkz.tkz_decode_batch_utf16(encoder, pi, po, batches.Count, pu, units.Length, poo, out needed);
                if (st == -4) { units = new char[needed]; continue; }              // TKZ_E_CAPACITY: `needed` is the exact size, in code units
                Tkz.Check(st);
                break;
            }
            var result = new List<string>(batches.Count);
            fixed (char* pu = units)
                for (int i = 0; i < batches.Count; ++i) result.Add(new string(pu, (int)outOffs[i], (int)(outOffs[i + 1] - outOffs[i])));
            return result;
        }

        /// <summary>Idempotent.  The pooled page-locked buffers go at once; a buffer set a call in flight holds is freed when that call returns it
        /// (ReturnBuffers), never under it; the native encoder goes when the last call that holds a reference on the SafeHandle has returned.</summary>
        public void Dispose()
        {
            disposed = true;
            while (bufferPool.TryTake(out PinnedBuffers b)) { b.Dispose(); GC.SuppressFinalize(b); }
            handle.Dispose();
        }
    }

    /// <summary>One rank of a sharded job (BASELINE configs[3]): rank r of `world` encodes documents tkz_shard_range(r) on its own GPU;
    /// the only exchange is one RCCL all-gather of {docs, bytes, tokens} per batch (tkz_comm_allgather_counts), from which every rank
    /// gets the global index of its first document and token; results go to one token shard file per rank (tkz_shard_write).
    /// The 128-byte communicator id travels from rank 0 to the others by whatever the host has (a file, a socket, MPI).</summary>
    public sealed class ShardedEncoder : IDisposable
    {
        private readonly IntPtr comm;
        public int Rank { get; }
        public int World { get; }
        public static byte[] NewCommunicatorId() { var id = new byte[128]; Tkz.Check(Tkz.tkz_comm_unique_id(id)); return id; }
        public ShardedEncoder(byte[] communicatorId, int rank, int world, int device)
        {
            Tkz.Check(Tkz.tkz_comm_create(communicatorId, rank, world, device, out comm));
            Rank = rank; World = world;
        }
        public (long Lo, long Hi) MyDocuments(long nDocsTotal) { Tkz.tkz_shard_range(nDocsTotal, Rank, World, out long lo, out long hi); return (lo, hi); }
        /// <summary>After encoding this rank's documents: exchange the counts, write the shard.  Returns the job totals {docs, bytes, tokens}.</summary>
        public long[] Publish(string shardPath, int[] ids, long nTokens, long[] offsets, long nDocs, long nBytes)
        {
            var table = new long[3 * World];
            Tkz.Check(Tkz.tkz_comm_allgather_counts(comm, nDocs, nBytes, nTokens, table));
            var bases = new long[3]; var totals = new long[3];
            Tkz.Check(Tkz.tkz_shard_bases(table, World, Rank, bases, totals));
            Tkz.Check(Tkz.tkz_shard_write(Tkz.Utf8Z(shardPath), ids, nTokens, offsets, nDocs, bases[0], bases[2]));
            return totals;
        }
        public void Dispose() { Tkz.tkz_comm_destroy(comm); }
    }
}
