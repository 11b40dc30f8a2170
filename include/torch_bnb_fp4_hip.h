/*
 * torch_bnb_fp4_hip.h -- C ABI of libtorch_bnb_fp4_hip.so, the MI355X (gfx950) FP4
 * dequant / fused-GEMV kernels.
 *
 * This is the drop-in boundary of the hot path: plain pointers and sizes, no torch
 * types.  Every pointer is a DEVICE pointer valid on the HIP device that is current
 * on the calling thread; `stream` is a hipStream_t (NULL = the null stream).  The
 * compute entry points are asynchronous (they enqueue on `stream` and return) and
 * re-entrant: they keep no state between calls and may be called from any number of
 * threads at once.  The only process-wide state is the benchmark hook
 * fp4_hip_set_variant() (relaxed atomics, read once per launch; a production caller
 * never touches it) and a per-device cache of the compute-unit count.
 * Return value: 0 on success, otherwise an fp4_status code; fp4_hip_last_error() then
 * holds a thread-local message.  The compute entry points neither allocate nor
 * synchronise, so every one of them is HIP-graph capturable.
 *
 * Each entry point names the reference interface it replaces
 * (aredden/torch-bnb-fp4, paths relative to that checkout).  The reference has no
 * C ABI of its own -- its boundary is the pybind module csrc/torch_fp4.cpp:125-139,
 * which torch-bnb-fp4_amd/csrc/torch_ext.cpp re-exports 1:1 on top of this header
 * (see INTEGRATION.md for the binding a reference maintainer would add).
 */
#ifndef TORCH_BNB_FP4_HIP_H
#define TORCH_BNB_FP4_HIP_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define FP4_HIP_ABI_VERSION 7
#define FP4_HIP_API __attribute__((visibility("default")))

/* Element types, numbered like the reference's ScalarTypeEnum (csrc/torch_fp4.cpp:22-26). */
enum fp4_dtype { FP4_DTYPE_F16 = 0, FP4_DTYPE_F32 = 1, FP4_DTYPE_BF16 = 2 };

/* Which 16-entry code table a dequant uses.
 * NF4      = bitsandbytes' NF4 code (see "NF4" below), nibble used as the index, no sign bit;
 * CODEBOOK = the CODE_PARAM literals (csrc/dequant_fp4_optimized.cu:28-46),
 * TREE     = the constants of dequantize_fp4_tree (csrc/dequant_fp4_optimized.cu:55-76);
 * they differ by 1-12 ulp in f32 for nibbles 1,4,6 (and 9,12,14). */
enum fp4_table { FP4_TABLE_CODEBOOK = 0, FP4_TABLE_TREE = 1, FP4_TABLE_NF4 = 2 };

/* Cache policy of the dequant's output stream.  AUTO = non-temporal loads and stores for large outputs (fastest
 * when the result is not read back at once: +30 % at 4096x4096); KEEP_CACHED = plain stores, for a consumer that
 * reads the weight right away (the dequant + GEMM of the batch > 1 path: the GEMM then hits L2 / Infinity Cache,
 * -2 us per 4096x4096 layer end to end); STREAM = always non-temporal. */
enum fp4_dequant_flags { FP4_DEQUANT_AUTO = 0, FP4_DEQUANT_KEEP_CACHED = 1, FP4_DEQUANT_STREAM = 2 };

enum fp4_status {
    FP4_OK = 0,
    FP4_ERR_INVALID_ARGUMENT = 1, /* null pointer, negative size, unknown enum */
    FP4_ERR_UNSUPPORTED = 2,      /* shape/blocksize the kernels do not cover */
    FP4_ERR_LAUNCH = 3            /* the HIP runtime failed: hipGetLastError() != hipSuccess after a launch, or a memset / sync of a host-side helper */
};

FP4_HIP_API int fp4_hip_abi_version(void);
FP4_HIP_API const char *fp4_hip_last_error(void);

/* Host-side copy of a code table (16 floats; CODEBOOK / TREE: nibble bit 3 = sign; NF4: plain index). */
FP4_HIP_API int fp4_hip_code_table(int table, float out16[16]);

/*
 * Blockwise FP4 -> f16 / bf16 / f32 dequant of n elements:
 *   out[e] = RN_T( f32(code[nibble(e)]) * absmax[e / blocksize] ),  0 <= e < n,
 * nibble(e) = HIGH nibble of packed[e/2] when e is even, LOW nibble when odd.
 * One f32 multiply, then round-to-nearest-even to T (f16 subnormals kept).
 *   packed : uint8[(n+1)/2]      absmax : float[ceil(n/blocksize)]      out : T[n]
 * blocksize: any even value >= 2 (power-of-two >= 32 takes the fast path).
 * Replaces dequantize_blockwise_fp4 (table = TREE, csrc/dequant_fp4_optimized.cu:182-205,
 * kernel :89-123) and dequantize_blockwise_codebook_fp4 (table = CODEBOOK, :207-255,
 * kernel :125-171).  Unlike the reference an unsupported dtype is an error, not a
 * printf (:201-203,250-252).
 */
FP4_HIP_API int fp4_hip_dequantize_blockwise(const uint8_t *packed, const float *absmax, void *out, int blocksize, int64_t n,
                                 int out_dtype, int table, int flags, void *stream);

/*
 * Fused batch-1 GEMV over an FP4 weight W[M,K] (row r = packed bytes [r*K/2, (r+1)*K/2),
 * scales absmax[(r*K + k) / blocksize]):
 *   out[r] = T( sum_k x[k] * code[nibble(r,k)] * absmax[(r*K+k)/blocksize] (+ bias[r]) )
 * accumulated in f32.  x, out, bias are T[K], T[M], T[M]; bias may be NULL.
 * With a bias the result is T( f32(T(sum)) + f32(bias[r]) ), i.e. exactly the
 * reference's separate `out += bias` (torch_bnb_fp4/__init__.py:608-613) fused in.
 * K must be even; K % 32 == 0 with a power-of-two blocksize >= 32 dividing K takes
 * the fast path (the reference's own GEMV gate, torch_bnb_fp4/__init__.py:593).
 * Replaces gemv_4bit_inference (csrc/gemv_fp4_optimized.cu:277-368; kernels :60-157
 * half/bf16 and :159-259 float).  The code values are those of the reference's GEMV, which ignores
 * its `datatype` tensor and uses CODE_PARAM (csrc/gemv_fp4_optimized.cu:266,274): the f32 kernels
 * read the bit-faithful CODE_PARAM f32 table; the f16 / bf16 kernels decode the exact k/12 values
 * (12 * |code| is exact in 16 bits, and CODE_PARAM rounded to f16 / bf16 - what the reference's
 * 16-bit kernels load, :92-96 - equals k/12 rounded to that type, tests/test_oracle.py), so the
 * two are indistinguishable there.
 */
FP4_HIP_API int fp4_hip_gemv(const void *x, const uint8_t *packed, const float *absmax, const void *bias, void *out, int64_t M,
                 int64_t K, int blocksize, int dtype, void *stream);

/*
 * The same GEMV with the elementwise work that FOLLOWS a Linear in a decoder layer folded into its epilogue, so that a
 * decode step pays one kernel boundary where the reference's op surface pays two to four
 * (torch_bnb_fp4/__init__.py:603-613 is where the reference already pays a separate launch for the bias).
 * Every intermediate is rounded to T exactly where the separate torch ops would round it:
 *   EPILOGUE_NONE:            t = T(sum_r); if bias: t = T(t + bias[r]); if residual: t = T(t + residual[r]); out[r] = t
 *                             out : T[M].  `residual` may alias `out` (h = h + Linear(a) in place).
 *   EPILOGUE_SILU_MUL_PAIRS:  the weight's rows interleave a gate and an up projection (row 2i = gate_i, row 2i+1 = up_i;
 *                             a row permutation done once at load time - rows of an FP4 weight are independent);
 *                             g = T(sum_2i) (+bias), u = T(sum_2i+1) (+bias), s = T(g / (1 + exp(-g))) (torch's silu),
 *                             t = T(s * u); if residual: t = T(t + residual[i]); out[i] = t.   out : T[M/2], M even.
 * 16-bit dtypes with K % 32 == 0 and a power-of-two blocksize >= 32 dividing K (the decode fast path) support both
 * epilogues; other shapes / f32 support EPILOGUE_NONE only and return FP4_ERR_UNSUPPORTED for the gated one, so the
 * caller can run the plain GEMV and the separate ops.  Not in the reference.
 *
 * At edge values every epilogue of this header (this entry point, the 2..128-row ones and the NF4, LoRA, multi-adapter and
 * nested forms) returns what those separate torch ops return on this device, value for value; a NaN is a NaN, payload and
 * sign unspecified.  Measured at every 16-bit gate pattern and at every call site (tests/test_gpu_epilogue_values.py):
 *   - s is the f32 FORMULA g / (1 + expf(-g)), not true silu.  A NaN gate gives NaN and so does g = -inf (-inf / inf);
 *     g = +inf gives +inf.  For g < -88.72 expf overflows and s is -0, where true silu would be a (tiny) normal number;
 *     from g = 16.64 on (expf(-g) <= 2^-24) 1 + e is 1 and s = g.  A sum or sum + bias beyond T's range makes the gate +-inf first.
 *   - bias and residual take part as ordinary rounded adds: a NaN or infinite bias or residual gives the NaN or infinity of
 *     IEEE addition (inf - inf and 0 * inf, through the up row, are NaN); a sum, add or product beyond T's largest value
 *     rounds to +-inf, ties go to even at every rounding.
 *   - signed zeros are IEEE's: -0 * u and s * -0 keep the sign of the product, x + -x is +0, -0 + -0 is -0; a sum of products
 *     that are all zero is +0 whatever their signs.
 *   - subnormals are kept everywhere: fp16 subnormals, and bf16 subnormals (f32 subnormals once widened), as gate, up row,
 *     bias, residual, sum and result; nothing is flushed.
 *   - the 16-bit FP4 kernels form f32(12 code x absmax) before the final * (1/12): a row sum whose magnitude passes
 *     f32 max / 12 = 2.8e37 (bf16 only) is +-inf although T could hold it.  The NF4 kernels and the f32 paths do not scale.
 */
enum fp4_epilogue { FP4_EPILOGUE_NONE = 0, FP4_EPILOGUE_SILU_MUL_PAIRS = 1 };
FP4_HIP_API int fp4_hip_gemv_fused(const void *x, const uint8_t *packed, const float *absmax, const void *bias, const void *residual,
                       void *out, int64_t M, int64_t K, int blocksize, int dtype, int epilogue, void *stream);

/*
 * Small-batch companion of the GEMV (2..128 activation rows; also accepts 1):
 *   out[b][r] = T( sum_k x[b][k] * code[nibble(r,k)] * absmax[(r*K+k)/blocksize] + bias[r] )
 * x is T[B,K] row-major, out T[B,M]; f32 accumulation, ONE rounding, bias added in f32 first (what the
 * reference's batch > 1 path, dequant + F.linear, does - torch_bnb_fp4/__init__.py:423-436,616-617 - without
 * writing and re-reading the M*K dequantised weight).  16-bit dtypes; f32 activations are covered up to 8 rows as B launches of the f32
 * GEMV (each row bit-identical to fp4_hip_gemv; FP4_ERR_UNSUPPORTED above that and for the gated epilogue).  Two kernels: a matrix-core one
 * (v_mfma_f32_16x16x32; blocksize 64, K % 512 == 0; any B <= 16) and a VALU one (B <= 8; K % 32 == 0, K <= 16384,
 * less for larger B; power-of-two blocksize >= 32 dividing K).  Returns FP4_ERR_UNSUPPORTED for shapes neither
 * covers, so the caller can fall back to dequant + GEMM.  17..64 rows (blocksize 64, K % 64 == 0; and 1..16 rows where
 * K % 512 != 0 keeps the two kernels above out, e.g. K = 11008): ONE pass over the
 * weight on the matrix cores with 2..4 column tiles of x per decoded weight fragment (x staged through LDS by LDS-DMA);
 * where that kernel does not apply the rows are split evenly over ceil(B/16) launches, each streaming the weight once.
 * 65..128 rows: two even chunks of at most 64.  Measured against dequant + hipBLASLt GEMM on MI355X
 * (profiles/r02_wide_batch_17_to_128_rows.txt): 1.7-3.1x faster at 17..64 rows, 1.27-1.6x at 65..128.
 * FP4_OK without a launch for B == 0 or M == 0; B > 128, a negative size or a null pointer: FP4_ERR_INVALID_ARGUMENT.  A refused
 * call (either error code) launches nothing and leaves out untouched - also at 17..128 rows, where every chunk has the same shape
 * and the first one is refused.
 */
FP4_HIP_API int fp4_hip_gemm_small(const void *x, const uint8_t *packed, const float *absmax, const void *bias, void *out,
                                   int64_t B, int64_t M, int64_t K, int blocksize, int dtype, void *stream);

/*
 * The small-batch product with the fused decode epilogues of fp4_hip_gemv_fused, for 1..128 activation rows (batched decode):
 *   EPILOGUE_NONE:            t = T(sum[b][r] + bias[r]) (F.linear: bias in f32, one rounding); if residual: t = T(t + residual[b][r])
 *                             out : T[B, M], residual : T[B, M].
 *   EPILOGUE_SILU_MUL_PAIRS:  rows interleave gate and up (row 2i / 2i+1): g = T(sum_2i + bias_2i), u = T(sum_2i+1 + bias_2i+1),
 *                             t = T(T(silu(g)) * u); if residual: t = T(t + residual[b][i]);  out, residual : T[B, M/2], M even.
 * `residual` may alias `out` under either epilogue (h = h + Linear(a) in place): on every path - the 16-row kernels, the one-pass
 * kernels, the 16-row and 64-row chunking - each output element is read and then written by the one thread that owns it.
 * Same shape coverage and FP4_ERR_UNSUPPORTED behaviour as fp4_hip_gemm_small; an unknown epilogue, or the gated one with an odd M
 * ("even row count"): FP4_ERR_INVALID_ARGUMENT.  Not in the reference.
 */
FP4_HIP_API int fp4_hip_gemm_small_fused(const void *x, const uint8_t *packed, const float *absmax, const void *bias,
                             const void *residual, void *out, int64_t B, int64_t M, int64_t K, int blocksize, int dtype,
                             int epilogue, void *stream);

/*
 * fp4_hip_gemm_small_fused with a caller-provided scratch buffer.  On short weights with long rows (M below 24 rows per CU, K >= 8192:
 * the down projection of a decoder) 33..64 activation rows (65..128: two even chunks) run as x-stationary split-K over workgroups: partial sums of 512-column
 * slices go through `workspace` and a second small launch adds them in a fixed order and applies the epilogue (deterministic, no
 * atomics).  fp4_hip_gemm_small_ws_bytes returns the bytes that path wants for a shape, or 0 where it would not be used (then, or
 * with workspace == NULL or too small, or with a blocksize other than 64, the call is exactly fp4_hip_gemm_small_fused).  16-byte aligned workspace; it may be reused by
 * the next call on the same stream; no byte beyond the returned size is written.  `residual` may alias `out` here too: the
 * reducing launch reads and writes each output element from one thread (the workspace must not overlap either).  Not in the reference.
 */
FP4_HIP_API int64_t fp4_hip_gemm_small_ws_bytes(int64_t B, int64_t M, int64_t K, int blocksize, int dtype);
FP4_HIP_API int fp4_hip_gemm_small_ws(const void *x, const uint8_t *packed, const float *absmax, const void *bias, const void *residual,
                          void *out, int64_t B, int64_t M, int64_t K, int blocksize, int dtype, int epilogue, void *workspace,
                          int64_t workspace_bytes, void *stream);

/*
 * K-split (row-parallel) building block: the same GEMV, but the f32 accumulator is written as is
 * (out_f32 : float[M], no bias, no rounding to T), so that the partial sums of the column shards
 * of one weight can be added across GPUs (RCCL all-reduce) before the single final rounding.
 * Not in the reference (it has no multi-GPU path); x is T[K] of x_dtype.
 */
FP4_HIP_API int fp4_hip_gemv_partial(const void *x, const uint8_t *packed, const float *absmax, float *out_f32, int64_t M,
                                     int64_t K, int blocksize, int x_dtype, void *stream);

/*
 * One-shot all-reduce for the K-split partials (the reference has no multi-GPU path).
 *
 * Setup (host side, synchronous, once): every rank allocates one slot buffer of fp4_hip_comm_bytes(world, capacity) bytes
 * with fp4_hip_comm_alloc (zero-filled device memory, uncached / fine-grained where the runtime offers it; `kind_out`
 * reports 0 uncached, 1 fine-grained, 2 plain), sends the 64-byte IPC handle to its peers by whatever channel the host
 * program has (torch.distributed all_gather in torch_bnb_fp4/comm.py) and maps theirs with fp4_hip_comm_open.
 *
 * fp4_hip_allreduce_oneshot(partial, peer_buffers, rank, world, M, capacity, bias, residual, out, dtype, timeout_us, stream):
 *   out[e] = T( T( T( sum_{p < world} partial_p[e] ) + bias[e] ) + residual[e] ),   e < M <= capacity,
 * the sum taken in f32 in rank order (identical bits on every rank).  `peer_buffers` is a HOST array of `world` device
 * pointers, entry `rank` being this rank's own buffer.  Each rank writes its partial as 8-byte {epoch, value} granules
 * straight into its slot of every peer's buffer (one hop over all xGMI links at once) and sweeps its own buffer until
 * all `world` slots carry the call's epoch; the epoch lives in device memory and slots are double-buffered, so the call
 * needs no host involvement and is HIP-graph capturable.  All ranks must issue their calls on a communicator in the
 * same order, one stream per rank.  Polling is bounded: after `timeout_us` (<= 0: 2 s) without a peer's data a lane
 * records {epoch, peer} in the buffer's status word and writes NaN; fp4_hip_comm_status copies {epoch, busy, status,
 * lanes timed out} to the host (synchronous) so the caller can raise.  The status word is sticky (first time-out wins) until
 * fp4_hip_comm_clear_status zeroes it and the lane count (synchronous; the epoch is kept, the call sequence continues), so that a
 * transient time-out is reported once and later checks speak about later calls.
 * Limit of that recovery: slots are double-buffered by call parity, so a rank that gave up on call n and carries on rewrites the slot of
 * call n at call n + 2.  A peer that lags by LESS than one call still finds its data; one that lags further meets a newer epoch in
 * the slot, times out in turn and writes NaN (never a wrong finite value).  Only the rank that timed out sees a status word - its peer
 * may hold a valid result for the same call - so the decision to go on must be taken by the whole group: reduce the status words
 * (MAX) over the ranks at the sync point and treat a non-zero result as a failure on every rank (OneShotAllReduce.check_collective).
 */
FP4_HIP_API int64_t fp4_hip_comm_bytes(int world, int64_t capacity);
FP4_HIP_API int fp4_hip_comm_alloc(int64_t bytes, void **ptr, uint8_t handle_out[64], int *kind_out);
FP4_HIP_API int fp4_hip_comm_open(const uint8_t handle[64], void **ptr);
FP4_HIP_API int fp4_hip_comm_close(void *ptr);
FP4_HIP_API int fp4_hip_comm_free(void *ptr);
FP4_HIP_API int fp4_hip_comm_status(const void *own_buffer, uint32_t out4[4]);
FP4_HIP_API int fp4_hip_comm_clear_status(void *own_buffer);
FP4_HIP_API int fp4_hip_allreduce_oneshot(const float *partial, void *const *peer_buffers, int rank, int world, int64_t M,
                              int64_t capacity, const void *bias, const void *residual, void *out, int out_dtype,
                              int64_t timeout_us, void *stream);

/*
 * Blockwise FP4 quantiser (the producer side; bitsandbytes' quantize_fp4 as called at
 * torch_bnb_fp4/__init__.py:775 and inside Params4bit.cuda(), :861):
 * per block of `blocksize` elements absmax = max|w|, code = nearest FP4 magnitude of
 * w/absmax (midpoint thresholds, strict >), sign in bit 3, even element in the high
 * nibble.  w is T[n] (w_dtype), packed uint8[(n+1)/2], absmax float[ceil(n/blocksize)].
 * blocksize: power of two, 32..4096.
 */
FP4_HIP_API int fp4_hip_quantize_blockwise(const void *w, int w_dtype, uint8_t *packed, float *absmax, int64_t n, int blocksize,
                               void *stream);

/*
 * NF4 -- bitsandbytes' second 4-bit code (quant_type "nf4"; QLoRA and most published bnb-4bit checkpoints).  Not in the
 * reference.  These entry points and FP4_TABLE_NF4 are additions to ABI version 7: nothing a v7 caller already uses changed.
 *   code (nibble 0..15, f32 rounding of the published decimals):
 *     -1.0, -0.6961928009986877, -0.5250730514526367, -0.39491748809814453, -0.28444138169288635, -0.18477343022823334,
 *     -0.09105003625154495, 0.0, 0.07958029955625534, 0.16093020141124725, 0.24611230194568634, 0.33791524171829224,
 *     0.44070982933044434, 0.5626170039176941, 0.7229568362236023, 1.0
 *   Packing and absmax as for FP4 (even element in the high nibble, one f32 scale per block).  Dequant:
 *   fp4_hip_dequantize_blockwise(..., table = FP4_TABLE_NF4, ...), out = RN_T(f32(code[nibble]) * absmax).
 *
 * fp4_hip_gemv_nf4: the batch-1 GEMV of fp4_hip_gemv over an NF4 weight; same arguments, shape coverage, bias rule
 * (T(f32(T(sum)) + f32(bias)) for 16-bit T) and error codes.  The f32 code values are used as they are (f32 accumulation).
 *   Non-finite activations (this entry point and fp4_hip_gemv_fused_nf4 / _lora_nf4 / _nested_nf4): a NaN or an infinite x[k] makes
 *   the outputs it enters non-finite - at batch 1 that is every out[r]; whether such an output is NaN or a signed infinity is
 *   unspecified (the fast path loads branch-free: lanes past the end of a row re-read its last 32 activations under a zero scale,
 *   so an infinity there also arrives as 0 * Inf).
 *
 * fp4_hip_quantize_blockwise_nf4: arguments as fp4_hip_quantize_blockwise.  absmax = max|w|, x = w * (1/absmax) in f32,
 *   nibble = #{ i : x > T[i] } over the 15 f32 midpoints T[i] = f32((code[i] + code[i+1]) / 2) (strict >; NaN -> 0, so an
 *   all-zero block, 0 * inf, is 0x00 bytes and dequantises to -0.0: what bitsandbytes writes).
 */
FP4_HIP_API int fp4_hip_gemv_nf4(const void *x, const uint8_t *packed, const float *absmax, const void *bias, void *out, int64_t M,
                                 int64_t K, int blocksize, int dtype, void *stream);
FP4_HIP_API int fp4_hip_quantize_blockwise_nf4(const void *w, int w_dtype, uint8_t *packed, float *absmax, int64_t n, int blocksize,
                                               void *stream);

/*
 * fp4_hip_gemm_small_nf4: fp4_hip_gemm_small over an NF4 weight, for 1..16 activation rows on the matrix cores:
 *   out[b][r] = T( sum_k x[b][k] * code[nibble(r,k)] * absmax[(r*K+k)/64] + bias[r] )       (bias optional; added in f32, ONE rounding)
 * Same argument conventions as fp4_hip_gemm_small.  The NF4 codes are exact in neither fp16 nor bf16, so every weight is fed to
 * v_mfma_f32_16x16x32 twice, as hi = T(code) and lo = T(code - hi) (fp16: lo * 2^24 in a tile of its own, so that no subnormal
 * input is relied on), both read from a 256-entry LDS table indexed by the packed byte; |hi + lo - code| <= 5.45e-6 |code|.
 * Covered: 1 <= B <= 16, blocksize 64, K % 512 == 0 (K <= 2^24), fp16 / bf16, any M >= 1 up to 2^30 (M * K may pass 2^32:
 * 64-bit addressing), x and packed 16-byte aligned.  Everything else: FP4_ERR_UNSUPPORTED, nothing launched, out untouched - the
 * caller uses NF4 dequant + GEMM.  FP4_OK without a launch for M == 0 or B == 0.  No 17+ rows; the fused epilogues are
 * fp4_hip_gemm_fused_nf4's.
 */
FP4_HIP_API int fp4_hip_gemm_small_nf4(const void *x, const uint8_t *packed, const float *absmax, const void *bias, void *out,
                                       int64_t B, int64_t M, int64_t K, int blocksize, int dtype, void *stream);

/*
 * fp4_hip_gemm_wide_nf4: the same product for 1..128 activation rows, one pass over the packed weight per at most 64 rows
 * (csrc/gemm_wide_nf4.hip): x is the A operand and the weight the B operand of v_mfma_f32_16x16x32, the hi / lo byte table of
 * fp4_hip_gemm_small_nf4 decodes, and every decoded fragment is multiplied with all ceil(B / 16) <= 4 column tiles of x.
 * f32 accumulation, bias added in f32, ONE rounding.  An addition to ABI version 7.
 * Covered: 1 <= B <= 128, blocksize 64, K % 64 == 0 (K <= 2^24), fp16 / bf16, any M >= 1 up to 2^30 (M * K may pass 2^32),
 * x and packed 16-byte aligned.  17..64 rows: one launch; 65..128 rows: two even chunks of at most 64 (two launches);
 * 1..16 rows: fp4_hip_gemm_small_nf4 itself where K % 512 == 0 (bit-identical), else the one-tile form of this kernel.
 * Deterministic (fixed summation order, no atomics), no allocation, no synchronisation: capturable.  Everything else:
 * FP4_ERR_UNSUPPORTED, nothing launched, out untouched.  FP4_OK without a launch for M == 0 or B == 0.  The fused epilogues are
 * fp4_hip_gemm_fused_nf4's.
 */
FP4_HIP_API int fp4_hip_gemm_wide_nf4(const void *x, const uint8_t *packed, const float *absmax, const void *bias, void *out,
                                      int64_t B, int64_t M, int64_t K, int blocksize, int dtype, void *stream);

/*
 * fp4_hip_gemv_fused_nf4: fp4_hip_gemv_fused over an NF4 weight - the batch-1 NF4 GEMV with the decode-step epilogues folded in,
 * every intermediate rounded to T where the separate torch ops would round it.  An addition to ABI version 7.
 *   EPILOGUE_NONE:            t = T(sum_r); if bias: t = T(t + bias[r]); if residual: t = T(t + residual[r]); out[r] = t.  out : T[M].
 *                             The sum is fp4_hip_gemv_nf4's, bit for bit (f32: plain f32 adds, sum + bias, then + residual).
 *   EPILOGUE_SILU_MUL_PAIRS:  rows 2i / 2i+1 are gate_i / up_i; g = T(sum_2i) (+bias), u = T(sum_2i+1) (+bias),
 *                             s = T(g / (1 + exp(-g))), t = T(s * u); if residual: t = T(t + residual[i]); out[i] = t.  out : T[M/2].
 * `residual` may alias `out`.  Covered: the fast path of fp4_hip_gemv_nf4 - K % 32 == 0, a power-of-two blocksize >= 32 dividing
 * K, x and packed 16-byte aligned; all three dtypes for EPILOGUE_NONE, fp16 / bf16 for the gated one.  Everything else:
 * FP4_ERR_UNSUPPORTED, nothing launched, out untouched - the caller runs fp4_hip_gemv_nf4 and the separate ops.  Unknown epilogue,
 * or the gated one with an odd M ("even row count"): FP4_ERR_INVALID_ARGUMENT.  FP4_OK without a launch for M == 0.
 */
FP4_HIP_API int fp4_hip_gemv_fused_nf4(const void *x, const uint8_t *packed, const float *absmax, const void *bias, const void *residual,
                                       void *out, int64_t M, int64_t K, int blocksize, int dtype, int epilogue, void *stream);

/*
 * fp4_hip_gemm_fused_nf4: fp4_hip_gemm_small_fused over an NF4 weight, with the coverage and the forwarding of
 * fp4_hip_gemm_wide_nf4 (1..128 rows, blocksize 64, K % 64 == 0, fp16 / bf16; 1..16 rows with K % 512 == 0 run the kernel of
 * fp4_hip_gemm_small_nf4; 65..128 rows are two even chunks).  Rounding is F.linear's, then the epilogue as separate rounded ops:
 *   EPILOGUE_NONE:            t = T(sum[b][r] + bias[r]); if residual: t = T(t + residual[b][r]).  out, residual : T[B, M].
 *                             With residual == NULL the result equals fp4_hip_gemm_wide_nf4's bit for bit.
 *   EPILOGUE_SILU_MUL_PAIRS:  g = T(sum_2i + bias_2i), u = T(sum_2i+1 + bias_2i+1), t = T(T(silu(g)) * u);
 *                             if residual: t = T(t + residual[b][i]).  out, residual : T[B, M/2], M even.
 * `residual` may alias `out`.  Deterministic, no allocation, no synchronisation: capturable.  Shapes outside the coverage:
 * FP4_ERR_UNSUPPORTED, nothing launched, out untouched.  Unknown epilogue, or the gated one with an odd M ("even row count"):
 * FP4_ERR_INVALID_ARGUMENT.  FP4_OK without a launch for M == 0 or B == 0.  An addition to ABI version 7.
 */
FP4_HIP_API int fp4_hip_gemm_fused_nf4(const void *x, const uint8_t *packed, const float *absmax, const void *bias, const void *residual,
                                       void *out, int64_t B, int64_t M, int64_t K, int blocksize, int dtype, int epilogue, void *stream);

/*
 * LoRA adapters beside an NF4 weight (QLoRA serving; an adapter cannot be merged into 4-bit weights without re-quantising them):
 *   y = W_nf4 x + B (s * A x)        A : T[R, K],  B : T[M, R],  s = lora_alpha / r.        Not in the reference.
 * Two steps, both accumulated in f32 in a fixed order (deterministic, no atomics), neither allocating nor synchronising (capturable).
 * Additions to ABI version 7.
 *
 * fp4_hip_lora_down: the down projection,
 *   t[b][j] = scale[j] * sum_k A[j][k] x[b][k],     written as f32 and never rounded to T.
 * x : T[Bt, K], A : T[R, K] row-major, scale : float[R] (one factor per adapter row, so stacked adapters may differ), t : float[Bt, R].
 * Covered: 1 <= Bt <= 64, R % 8 == 0 with 8 <= R <= 256 (pad A with zero rows), K % 8 == 0 (K <= 2^24), fp16 / bf16 / f32,
 * x and A 16-byte aligned.  Everything else: FP4_ERR_UNSUPPORTED, nothing launched, t untouched.  FP4_OK without a launch for Bt == 0.
 * A NaN or an infinite x[b][k] makes every t[b][j] of its own row b non-finite and touches no other row; NaN versus a signed infinity
 * is unspecified (units past the end of K re-read the row's last 8 activations against a zeroed A: 0 * Inf).
 *
 * fp4_hip_gemv_lora_nf4 / fp4_hip_gemm_lora_nf4: fp4_hip_gemv_fused_nf4 / fp4_hip_gemm_fused_nf4 with the adapter term
 *   delta[b][r] = sum_j f32(lora_B[r][j]) * t[b][j]
 * added to the kernel's f32 row sum BEFORE anything is rounded (sum' = sum + delta, one f32 add); everything after that is the
 * epilogue of the plain entry point, unchanged:
 *   batch 1 (gemv):  T(sum'), then T(+ bias), then T(+ residual);         2+ rows (gemm):  T(sum' + bias), then T(+ residual);
 *   EPILOGUE_SILU_MUL_PAIRS: the same change to the gate row and to the up row before their rounding.
 * That is one rounding fewer than adding a separately rounded adapter output.  With lora_B == 0 or t == 0 the result equals the plain
 * fused entry point's, value for value.  lora_B : T[M, R] row-major over the weight's own row order (for a gate|up weight: rows
 * interleaved like the weight's), t : float[B, R] as written by fp4_hip_lora_down (float[R] for the GEMV), R as above.
 * Covered: what fp4_hip_gemv_fused_nf4 covers (all three dtypes for EPILOGUE_NONE, fp16 / bf16 for the gated one), respectively
 * what fp4_hip_gemm_fused_nf4 covers up to 64 rows; R % 8 == 0 with 8 <= R <= 256; lora_B and t 16-byte aligned.  Everything else:
 * FP4_ERR_UNSUPPORTED, nothing launched, out untouched - the caller runs the plain fused op and adds the adapter separately.
 * Unknown epilogue, the gated one with an odd M ("even row count"), a negative size: FP4_ERR_INVALID_ARGUMENT.  FP4_OK without a
 * launch for M == 0 (or B == 0).  `residual` may alias `out`.
 */
FP4_HIP_API int fp4_hip_lora_down(const void *x, const void *A, const float *scale, float *t, int64_t Bt, int64_t R, int64_t K, int dtype,
                                  void *stream);
FP4_HIP_API int fp4_hip_gemv_lora_nf4(const void *x, const uint8_t *packed, const float *absmax, const void *bias, const void *residual,
                                      const void *lora_B, const float *t, int64_t R, void *out, int64_t M, int64_t K, int blocksize,
                                      int dtype, int epilogue, void *stream);
FP4_HIP_API int fp4_hip_gemm_lora_nf4(const void *x, const uint8_t *packed, const float *absmax, const void *bias, const void *residual,
                                      const void *lora_B, const float *t, int64_t R, void *out, int64_t B, int64_t M, int64_t K,
                                      int blocksize, int dtype, int epilogue, void *stream);

/*
 * Several adapters in one batch, selected per activation row on the device (sequence 0 one tenant's fine-tune, sequence 1 another's,
 * sequence 2 the bare base model): still one pass over the packed weight per step, whatever the mix.  Not in the reference.
 * Additions to ABI version 7.  All device memory:
 *   A_stack : T[n_adapters][R][K]        the single-adapter A arrays one after another
 *   B_stack : T[n_adapters][M][R]        over the weight's own row order (interleaved for a gate|up weight)
 *   scale_stack : float[n_adapters][R]   ids : int32[rows], the adapter of each activation row
 * An id outside 0 .. n_adapters - 1 (negative values included) means "no adapter for this row"; no address is formed from such an
 * id.  ids is read on the device only - no host read, no synchronisation - so a captured step follows an in-place rewrite of ids.
 * The slice offsets id * R * K and id * M * R are 64-bit.  Adapters of different ranks are zero-padded to one R (exact).
 *
 * fp4_hip_lora_down_multi: t[b][j] = scale_stack[a][j] * sum_k A_stack[a][j][k] x[b][k] with a = ids[b]; a row without an adapter
 * gets t[b][:] = +0.0f (written, not skipped).  Row b is bit-identical to row b of fp4_hip_lora_down(x, A_stack[a], scale_stack[a], ..)
 * on the same x.  Coverage and error codes are fp4_hip_lora_down's (A_stack 16-byte aligned; K % 8 == 0 aligns every slice; at most
 * 2^20 adapters); in addition n_adapters < 1 or a null ids is FP4_ERR_INVALID_ARGUMENT.  The A fragment is reloaded only when a row's
 * adapter differs from the previous row's, so a batch sorted by adapter reads A as often as the single-adapter kernel does.
 *
 * fp4_hip_gemm_lora_multi_nf4: the coverage of fp4_hip_gemm_lora_nf4 (1..64 rows, blocksize 64, K % 64 == 0, fp16 / bf16, both
 * epilogues, `residual` may alias `out`).  A row with adapter a is bit-identical to the same row of fp4_hip_gemm_lora_nf4 called with
 * B_stack[a] and the same t; a row without one is bit-identical to the same row of fp4_hip_gemm_fused_nf4 - the add is skipped, not
 * done with zero, so a -0 sum keeps its sign.  The gated epilogue applies the same rule to the gate row and the up row.
 * t : float[B, R] (fp4_hip_lora_down_multi's output).
 *
 * fp4_hip_gemv_lora_multi_nf4: the same for one row (ids : int32[1], t : float[R]): bit-identical to fp4_hip_gemv_lora_nf4 with the
 * slice ids[0] names, or to fp4_hip_gemv_fused_nf4 where it names none - so that a captured one-row step follows ids as well.
 *
 * Both: n_adapters < 1 or a null ids is FP4_ERR_INVALID_ARGUMENT; B_stack and t 16-byte aligned, R % 8 == 0 in 8..256, else
 * FP4_ERR_UNSUPPORTED with nothing launched and out untouched, as for the single-adapter forms.
 */
FP4_HIP_API int fp4_hip_lora_down_multi(const void *x, const void *A_stack, const float *scale_stack, const int32_t *ids, float *t,
                                        int64_t Bt, int64_t n_adapters, int64_t R, int64_t K, int dtype, void *stream);
FP4_HIP_API int fp4_hip_gemm_lora_multi_nf4(const void *x, const uint8_t *packed, const float *absmax, const void *bias,
                                            const void *residual, const void *B_stack, const int32_t *ids, int64_t n_adapters,
                                            const float *t, int64_t R, void *out, int64_t B, int64_t M, int64_t K, int blocksize,
                                            int dtype, int epilogue, void *stream);
FP4_HIP_API int fp4_hip_gemv_lora_multi_nf4(const void *x, const uint8_t *packed, const float *absmax, const void *bias,
                                            const void *residual, const void *B_stack, const int32_t *ids, int64_t n_adapters,
                                            const float *t, int64_t R, void *out, int64_t M, int64_t K, int blocksize, int dtype,
                                            int epilogue, void *stream);

/*
 * Nested (double-quantised) absmax -- bitsandbytes' compress_statistics (bnb_4bit_use_double_quant=True, the QLoRA recipe): the
 * per-block scales of a 4-bit weight are themselves quantised.  Per weight with nb = ceil(M*K / blocksize) blocks and g = nested_blocksize:
 *   absmax_u8 : uint8[nb]      nested_absmax : float[ceil(nb / g)]      code256 : float[256]      offset : one float
 *   absmax[i] = fl32( fl32( code256[absmax_u8[i]] * nested_absmax[i / g] ) + offset )        a multiply, then an add: two roundings.
 * Not in the reference.  Additions to ABI version 7.  All three are deterministic, neither allocate nor synchronise, and take
 * `offset` by value (no host scalar is read on the device): capturable.
 *
 * fp4_hip_absmax_unnest: writes the nb expanded scales to out_f32, after which every entry point above applies unchanged.
 *   g: a power of two in 64..4096 (else FP4_ERR_UNSUPPORTED); nb <= 2^31; the last group may be partial; FP4_OK without a launch
 *   for nb == 0; a null pointer or nb < 0: FP4_ERR_INVALID_ARGUMENT.  Nothing is launched and out is untouched on an error.
 *
 * fp4_hip_absmax_nest: the writing side.  Per group: v = fl32(a - offset), m = max|v|, n = fl32(v * fl32(1 / m)),
 *   out_u8 = the index of the entry of code256 nearest to n (an exact tie: the lower index), out_nested_absmax = m.  A group with
 *   m == 0 gets every out_u8 = the index of the table's 0.0, so it expands to exactly `offset`.  Any offset is valid (bitsandbytes
 *   uses the mean of absmax); the table needs no particular order.  Same argument rules as fp4_hip_absmax_unnest.
 *
 * fp4_hip_gemv_nested_nf4: fp4_hip_gemv_fused_nf4 reading the compressed statistics directly (33 instead of 36 bytes streamed per
 *   64 weights at blocksize 64, and a quarter of the resident statistics).  The scale is formed by the formula above inside the
 *   kernel; everything after it is fp4_hip_gemv_fused_nf4's, so the result EQUALS fp4_hip_gemv_fused_nf4 on the expanded absmax
 *   bit for bit, for every shape, dtype and epilogue.  Covered: what fp4_hip_gemv_fused_nf4 covers, with nested_blocksize == 256
 *   (what every bitsandbytes file holds).  Everything else: FP4_ERR_UNSUPPORTED, nothing launched, out untouched - the caller
 *   expands the statistics and runs the plain entry points.  Error codes otherwise as fp4_hip_gemv_fused_nf4; nested_blocksize <= 0
 *   or a null nested_absmax / code256: FP4_ERR_INVALID_ARGUMENT.
 *
 * fp4_hip_gemm_nested_nf4: fp4_hip_gemm_fused_nf4 reading the compressed statistics directly - the same rows (1..128), shapes,
 *   forwarding rule (1..16 rows with K % 512 == 0: the small-batch kernel, else the wide one, two chunks above 64 rows) and
 *   epilogues; `residual` may alias `out`.  The kernels fetch the block's code and its group's scale where they fetched the f32
 *   scale and form it by the formula above; everything after it is unchanged, so the result EQUALS fp4_hip_gemm_fused_nf4 on the
 *   expanded absmax bit for bit.  Covered: what fp4_hip_gemm_fused_nf4 covers (blocksize 64, K % 64 == 0, fp16 / bf16), with
 *   nested_blocksize == 256.  Everything else: FP4_ERR_UNSUPPORTED, nothing launched, out untouched - the caller expands the
 *   statistics with fp4_hip_absmax_unnest and runs fp4_hip_gemm_fused_nf4.  nested_blocksize <= 0, a null operand with M, K > 0, an
 *   unknown epilogue: FP4_ERR_INVALID_ARGUMENT.
 *
 * fp4_hip_gemv_lora_nested_nf4 / fp4_hip_gemm_lora_nested_nf4: fp4_hip_gemv_lora_nf4 / fp4_hip_gemm_lora_nf4 (one adapter, 1 row /
 *   1..64 rows) reading the compressed statistics, bit for bit equal to them on the expanded absmax; coverage and error codes are
 *   theirs, with the rules for the statistics above.
 */
FP4_HIP_API int fp4_hip_absmax_unnest(const uint8_t *absmax_u8, const float *nested_absmax, const float *code256, float offset,
                                      int nested_blocksize, int64_t nb, float *out_f32, void *stream);
FP4_HIP_API int fp4_hip_absmax_nest(const float *absmax_f32, int64_t nb, float offset, const float *code256, int nested_blocksize,
                                    uint8_t *out_u8, float *out_nested_absmax, void *stream);
FP4_HIP_API int fp4_hip_gemv_nested_nf4(const void *x, const uint8_t *packed, const uint8_t *absmax_u8, const float *nested_absmax,
                                        const float *code256, float offset, int nested_blocksize, const void *bias, const void *residual,
                                        void *out, int64_t M, int64_t K, int blocksize, int dtype, int epilogue, void *stream);
FP4_HIP_API int fp4_hip_gemm_nested_nf4(const void *x, const uint8_t *packed, const uint8_t *absmax_u8, const float *nested_absmax,
                                        const float *code256, float offset, int nested_blocksize, const void *bias, const void *residual,
                                        void *out, int64_t B, int64_t M, int64_t K, int blocksize, int dtype, int epilogue, void *stream);
FP4_HIP_API int fp4_hip_gemv_lora_nested_nf4(const void *x, const uint8_t *packed, const uint8_t *absmax_u8, const float *nested_absmax,
                                             const float *code256, float offset, int nested_blocksize, const void *bias,
                                             const void *residual, const void *lora_B, const float *t, int64_t R, void *out, int64_t M,
                                             int64_t K, int blocksize, int dtype, int epilogue, void *stream);
FP4_HIP_API int fp4_hip_gemm_lora_nested_nf4(const void *x, const uint8_t *packed, const uint8_t *absmax_u8, const float *nested_absmax,
                                             const float *code256, float offset, int nested_blocksize, const void *bias,
                                             const void *residual, const void *lora_B, const float *t, int64_t R, void *out, int64_t B,
                                             int64_t M, int64_t K, int blocksize, int dtype, int epilogue, void *stream);

/*
 * Tuning hook for benchmarks/sweeps: selects a kernel geometry by name
 * ("dequant", "gemv", "gemv_nf4" (0 = 16-entry f32 table, 1 = 256-entry pair table), "gemm_wide_nf4" (1 / 2 = 16 / 32 weight rows per workgroup), "gemm_small", "gemm_wide" = rows per workgroup of the 17..64-row kernels (1 / 2 / 3 / 4 = 16 / 32 / 64 / 128, 5 = 16 with self-contained waves; 0 = off),
 * "quantize": 1..999 = the persistent kernel with that many workgroups per CU, 1001 / 1002 / 1004 = the one-shot tiles kernel with 1 / 2 / 4 loads per lane).  variant < 0 (quantize: 0) restores the built-in heuristic.
 * Process-wide (relaxed atomics: safe to flip while other threads launch, each launch
 * reads it once); for sweeps and tests only, not part of the reference surface.
 */
FP4_HIP_API int fp4_hip_set_variant(const char *kernel, int variant);

#ifdef __cplusplus
}
#endif
#endif /* TORCH_BNB_FP4_HIP_H */
