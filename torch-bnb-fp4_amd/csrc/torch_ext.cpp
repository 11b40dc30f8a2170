// torch_bnb_fp4_ext -- the PyTorch-ROCm host layer above the C ABI (include/torch_bnb_fp4_hip.h).
//
// Re-exports the operator surface of the reference's pybind module (reference
// csrc/torch_fp4.cpp:125-139): ScalarType + dequantize_fp4, dequantize_fp4_codebook, gemv_fp4,
// qlinear, qlinear_bias, qlinear_codebook, qlinear_codebook_bias, with the same positional
// signatures, argument meaning and error behaviour (RuntimeError on a non-GPU / non-contiguous
// tensor, TypeError on a bad enum).  PyTorch is plumbing only: it owns device memory and the current
// stream; the batch>1 GEMM is a plain library GEMM on hipBLASLt, called directly with cached plans
// (lt_linear below; at::linear is its fallback); every FP4 kernel is behind the C ABI.
// Differences from the reference, all deliberate:
//   * launches go to the CURRENT torch stream under a device guard (the reference uses the legacy
//     default stream and no guard, csrc/dequant_fp4_optimized.cu:176, csrc/gemv_fp4_optimized.cu:266);
//   * launch / dtype failures raise instead of printf (csrc/dequant_fp4_optimized.cu:48-53,201-203);
//   * qlinear_codebook* dequantise all M*N elements (the reference passes the BYTE count,
//     csrc/torch_fp4.cpp:90,101, leaving half of the weight uninitialised).
// Extra exports (not in the reference):
//   * FP4:    gemv_fp4_bias, gemv_fp4_fused, gemm_small_fp4, gemm_small_fp4_fused, gemv_fp4_partial, quantize_fp4;
//   * NF4 (bitsandbytes' second 4-bit code, same shapes and dispatch): dequantize_nf4, gemv_nf4, gemv_nf4_bias, qlinear_nf4,
//     qlinear_nf4_bias, gemm_small_nf4, gemm_wide_nf4, gemv_nf4_fused, gemm_nf4_fused, quantize_nf4;
//   * LoRA adapters beside an NF4 weight: lora_down, gemv_nf4_lora, gemm_nf4_lora; several adapters per batch, chosen per row on
//     the device: lora_down_multi, gemv_nf4_lora_multi, gemm_nf4_lora_multi;
//   * double-quantised absmax: absmax_unnest, absmax_nest, gemv_nf4_nested, gemm_nf4_nested, gemv_nf4_lora_nested,
//     gemm_nf4_lora_nested, qlinear_nf4_nested;
//   * tensor parallelism: comm_alloc / comm_open / comm_close / comm_free / comm_status / comm_clear_status, allreduce_oneshot;
//   * hooks: code_table, set_kernel_variant, set_qlinear_gemm, qlinear_gemm_stats.
// The fused 4-bit weight ops (every *_fused, gemm_small_*, gemm_wide_nf4, *_lora, gemv_nf4_nested, gemv_fp4_partial) validate their
// operands in one place, weight_op() below.
#include <ATen/autocast_mode.h>
#include <ATen/core/grad_mode.h>
#include <c10/core/DeviceGuard.h>
#include <c10/hip/HIPStream.h>
#include <hip/hip_runtime_api.h>
#include <hipblaslt/hipblaslt.h>
#include <torch/extension.h>

#include <atomic>
#include <cstdint>
#include <cstdlib>
#include <mutex>
#include <stdexcept>
#include <string>
#include <tuple>
#include <unordered_map>
#include <utility>
#include <vector>

#include "torch_bnb_fp4_hip.h"

namespace {

enum class ScalarTypeEnum { float16 = FP4_DTYPE_F16, float32 = FP4_DTYPE_F32, bfloat16 = FP4_DTYPE_BF16 };

torch::ScalarType to_torch(ScalarTypeEnum t) {
    switch (t) {
        case ScalarTypeEnum::float16:
            return torch::kFloat16;
        case ScalarTypeEnum::float32:
            return torch::kFloat32;
        case ScalarTypeEnum::bfloat16:
            return torch::kBFloat16;
    }
    throw py::type_error("Unsupported scalar type");
}

int to_fp4_dtype(torch::ScalarType t, const char *what) {
    switch (t) {
        case torch::kFloat16:
            return FP4_DTYPE_F16;
        case torch::kFloat32:
            return FP4_DTYPE_F32;
        case torch::kBFloat16:
            return FP4_DTYPE_BF16;
        default:
            TORCH_CHECK(false, what, ": unsupported dtype ", t, " (need float16, bfloat16 or float32)");
    }
}

void check_gpu_contiguous(const torch::Tensor &t, const char *name, const char *op = nullptr) {
    // reference: CHECK_CUDA / CHECK_CONTIGUOUS (csrc/torch_fp4.cpp:19-20); the ops beyond the reference's name themselves
    const char *prefix = op ? op : "", *sep = op ? ": " : "";
    TORCH_CHECK(t.is_cuda(), prefix, sep, name, " must be a CUDA tensor");
    TORCH_CHECK(t.is_contiguous(), prefix, sep, name, " must be contiguous");
}

void check_on_device(const char *op, const char *name, const torch::Tensor &t, const torch::Tensor &A) {
    TORCH_CHECK(t.device() == A.device(), op, ": ", name, " is on ", t.device(), ", the activation on ", A.device(),
                "; all tensors must be on one device");
}

// an optional epilogue operand (bias, residual): `n` elements of `st` on `device`; `keep` holds the contiguous tensor the pointer is of
const void *epilogue_operand(const char *op, const char *name, const c10::optional<torch::Tensor> &t, int64_t n, torch::ScalarType st,
                             const torch::Device &device, torch::Tensor &keep) {
    if (!t.has_value()) return nullptr;
    TORCH_CHECK(t->is_cuda() && t->numel() == n && t->scalar_type() == st && t->device() == device, op, ": ", name, " must hold ", n,
                " elements of dtype ", st, " on the activation's device (", device, "); got ", t->numel(), " of ", t->scalar_type(), " on ",
                t->device());
    keep = t->contiguous();
    return keep.data_ptr();
}

void check_status(int rc) {
    if (rc == FP4_OK) return;
    const std::string msg = fp4_hip_last_error();
    // the reference's wording for a dtype its kernels do not take (csrc/gemv_fp4_optimized.cu:362-363) - for the entry points' dtype
    // refusals only ("<entry point>: unsupported dtype <n>"), not for every message that prints a dtype=<n> among the shape it refuses
    if (rc == FP4_ERR_UNSUPPORTED && msg.find("unsupported dtype ") != std::string::npos) throw std::runtime_error("Unsupported datatype: " + msg);
    TORCH_CHECK(false, msg);
}

void *current_stream(const torch::Tensor &t) { return c10::hip::getCurrentHIPStream(t.device().index()).stream(); }

// dequant of the first n elements of `out` (out is [M,N], n <= M*N)
void dequant_into(const torch::Tensor &A, const torch::Tensor &absmax, torch::Tensor &out, int64_t blocksize, int64_t n,
                  int table, int flags = FP4_DEQUANT_AUTO) {
    // reference: TORCH_CHECKs of csrc/dequant_fp4_optimized.cu:183-187,210-213
    TORCH_CHECK(A.dtype() == torch::kUInt8, "A must be uint8");
    TORCH_CHECK(absmax.dtype() == torch::kFloat32, "absmax must be float32");
    TORCH_CHECK(A.is_cuda(), "A must be cuda");
    TORCH_CHECK(absmax.is_cuda(), "absmax must be cuda");
    TORCH_CHECK(out.is_cuda(), "out must be cuda");
    TORCH_CHECK(absmax.device() == A.device() && out.device() == A.device(), "A, absmax and out must be on one device");
    TORCH_CHECK(n >= 0 && n <= out.numel(), "n = ", n, " does not fit the [M, N] output (", out.numel(), " elements)");
    TORCH_CHECK(blocksize >= 2 && blocksize % 2 == 0, "blocksize must be even and >= 2");
    TORCH_CHECK(A.numel() >= (n + 1) / 2, "packed tensor holds ", A.numel(), " bytes, ", (n + 1) / 2, " needed");
    TORCH_CHECK(absmax.numel() >= (n + blocksize - 1) / blocksize, "absmax holds ", absmax.numel(), " scales, ",
                (n + blocksize - 1) / blocksize, " needed");
    const int dt = to_fp4_dtype(out.scalar_type(), "dequantize");
    c10::DeviceGuard guard(A.device());
    check_status(fp4_hip_dequantize_blockwise(A.data_ptr<uint8_t>(), absmax.data_ptr<float>(), out.data_ptr(), (int)blocksize,
                                              n, dt, table, flags, current_stream(A)));
}

torch::Tensor dequantize_impl(const torch::Tensor &A, const torch::Tensor &absmax, int blocksize, int M, int N, int64_t n,
                              ScalarTypeEnum o_type, int table) {
    check_gpu_contiguous(A, "A");
    check_gpu_contiguous(absmax, "absmax");
    torch::Tensor out = torch::empty({M, N}, torch::TensorOptions().dtype(to_torch(o_type)).device(A.device()));
    dequant_into(A, absmax, out, blocksize, n, table);
    return out;
}

torch::Tensor dequantize_fp4(torch::Tensor A, torch::Tensor absmax, int blocksize, int M, int N, ScalarTypeEnum o_type) {
    return dequantize_impl(A, absmax, blocksize, M, N, int64_t(M) * N, o_type, FP4_TABLE_TREE);
}

// the `codebook` tensor of the *_codebook ops is checked at most and never read, like the reference's (its kernels use CODE_PARAM)
torch::Tensor dequantize_fp4_codebook(torch::Tensor A, torch::Tensor absmax, torch::Tensor codebook, int M, int N,
                                      int blocksize, int64_t n, ScalarTypeEnum dtype) {
    check_gpu_contiguous(A, "A");
    check_gpu_contiguous(absmax, "absmax");
    check_gpu_contiguous(codebook, "codebook");
    return dequantize_impl(A, absmax, blocksize, M, N, n, dtype, FP4_TABLE_CODEBOOK);
}

torch::Tensor dequantize_nf4(torch::Tensor A, torch::Tensor absmax, int blocksize, int M, int N, ScalarTypeEnum o_type) {
    return dequantize_impl(A, absmax, blocksize, M, N, int64_t(M) * N, o_type, FP4_TABLE_NF4);
}

// ---- the dense GEMM of the batch > 1 path: hipBLASLt, called directly ------------------------------------------------------------
// The reference's batch > 1 path is dequant + torch::nn::functional::linear (csrc/torch_fp4.cpp:64-103).  On ROCm every torch GEMM
// entry point (linear, addmm, mm, with or without bias, either BLAS backend) costs ~18.5 us of HOST time per call on this platform
// (tools/exp_blas_host_cost.py; a trivial torch op: 4.3 us), most of it descriptor set-up and the heuristic query repeated on every
// call - and an eager small-batch forward is host-bound, so the dequant + GEMM layer came out slower than the dense layer it replaces
// (BASELINE config 3, `c3_sanity_mlp`).  The same library call with the descriptors, layouts and the chosen algorithm cached per
// (device, dtype, rows, M, K, bias) costs a few microseconds.  Same maths as at::linear: x [rows, K] row-major times W [M, K]^T,
// f32 accumulation (HIPBLAS_COMPUTE_32F, no reduced-precision f32 mode), bias through the library's epilogue, one rounding to T.
// Anything this path does not cover - other dtypes, a bias of another dtype, no algorithm returned, the first call of a device
// arriving under stream capture - goes to at::linear; FP4_QLINEAR_GEMM=aten (or set_qlinear_gemm("aten")) forces that route.
// The library call is a product and nothing else: it records no autograd node and knows no cast policy.  Where at::linear means
// more than the product the direct route steps aside (qlinear_impl): grad mode on with an activation or a bias that requires
// grad (the reference's F.linear sends gradient to both), or autocast enabled for the activation's device type.  no_grad,
// inference_mode and inputs that do not require grad keep the direct route.  qlinear_gemm_stats() counts the calls each route
// served, process-wide (no reset: take differences).
std::atomic<int> g_qlinear_gemm{-1};  // -1 = not decided yet (environment), 0 = at::linear, 1 = hipBLASLt direct
std::atomic<uint64_t> g_qlinear_direct_calls{0}, g_qlinear_aten_calls{0};

py::dict qlinear_gemm_stats() {
    py::dict d;
    d["direct"] = g_qlinear_direct_calls.load(std::memory_order_relaxed);
    d["aten"] = g_qlinear_aten_calls.load(std::memory_order_relaxed);
    return d;
}

bool qlinear_gemm_direct() {
    int v = g_qlinear_gemm.load(std::memory_order_relaxed);
    if (v < 0) {
        const char *e = std::getenv("FP4_QLINEAR_GEMM");
        v = (e && std::string(e) == "aten") ? 0 : 1;
        g_qlinear_gemm.store(v, std::memory_order_relaxed);
    }
    return v == 1;
}

std::string set_qlinear_gemm(const std::string &which) {
    TORCH_CHECK(which == "hipblaslt" || which == "aten", "set_qlinear_gemm: 'hipblaslt' or 'aten', got '", which, "'");
    const bool was = qlinear_gemm_direct();
    g_qlinear_gemm.store(which == "hipblaslt" ? 1 : 0, std::memory_order_relaxed);
    return was ? "hipblaslt" : "aten";
}

struct LtPlan {
    hipblasLtMatmulDesc_t desc = nullptr;
    hipblasLtMatrixLayout_t a = nullptr, b = nullptr, c = nullptr;
    hipblasLtMatmulAlgo_t algo{};
    size_t workspace = 0;
    bool usable = false;
    ~LtPlan() {
        if (a) hipblasLtMatrixLayoutDestroy(a);
        if (b) hipblasLtMatrixLayoutDestroy(b);
        if (c) hipblasLtMatrixLayoutDestroy(c);
        if (desc) hipblasLtMatmulDescDestroy(desc);
    }
};

struct LtKey {
    int device, dtype, bias;
    int64_t rows, M, K;
    bool operator==(const LtKey &o) const {
        return device == o.device && dtype == o.dtype && bias == o.bias && rows == o.rows && M == o.M && K == o.K;
    }
};
struct LtKeyHash {
    size_t operator()(const LtKey &k) const {
        size_t h = std::hash<int64_t>()(k.rows * 1000003 + k.M);
        h ^= std::hash<int64_t>()(k.K * 31 + k.dtype * 7 + k.bias * 3 + k.device) + 0x9e3779b97f4a7c15ULL + (h << 6) + (h >> 2);
        return h;
    }
};

// one handle per device, shared by every thread (hipblasLtMatmul is thread-safe on a handle as long as the workspaces differ)
hipblasLtHandle_t lt_handle(int device, bool may_create) {
    static std::mutex mu;
    static hipblasLtHandle_t handles[64] = {};
    if (device < 0 || device >= 64) return nullptr;
    std::lock_guard<std::mutex> lock(mu);
    if (!handles[device] && may_create) {
        hipblasLtHandle_t h = nullptr;
        if (hipblasLtCreate(&h) == HIPBLAS_STATUS_SUCCESS) handles[device] = h;
    }
    return handles[device];
}

constexpr size_t kLtMaxWorkspace = size_t(76) << 20;  // what torch itself grants hipBLASLt on gfx94x / gfx95x: the heuristic then picks from the same algorithms

// Plans are per THREAD: the bias pointer is an attribute of the matmul descriptor and is set on every call, so a descriptor must not
// be shared by two threads launching at once (the concurrency promise of this boundary: tests/test_gpu_concurrency.py).
LtPlan *lt_plan(hipblasLtHandle_t handle, const LtKey &key, hipDataType dt) {
    thread_local std::unordered_map<LtKey, std::unique_ptr<LtPlan>, LtKeyHash> plans;
    auto it = plans.find(key);
    if (it != plans.end()) return it->second.get();
    // (a prefill loop over ever-changing sequence lengths must not grow this without bound: plans are cheap to rebuild, ~0.1 ms each)
    if (plans.size() >= 4096) plans.clear();
    auto plan = std::make_unique<LtPlan>();
    LtPlan *p = plan.get();
    plans.emplace(key, std::move(plan));  // kept even if unusable: the failure is remembered, not retried on every call
    // column-major view of the row-major operands: D[M, rows] = op_T(A = W as K x M, ld K) * (B = x as K x rows, ld K), ld(D) = M
    const hipblasOperation_t opT = HIPBLAS_OP_T, opN = HIPBLAS_OP_N;
    if (hipblasLtMatmulDescCreate(&p->desc, HIPBLAS_COMPUTE_32F, HIP_R_32F) != HIPBLAS_STATUS_SUCCESS) return p;
    if (hipblasLtMatmulDescSetAttribute(p->desc, HIPBLASLT_MATMUL_DESC_TRANSA, &opT, sizeof(opT)) != HIPBLAS_STATUS_SUCCESS ||
        hipblasLtMatmulDescSetAttribute(p->desc, HIPBLASLT_MATMUL_DESC_TRANSB, &opN, sizeof(opN)) != HIPBLAS_STATUS_SUCCESS)
        return p;
    if (key.bias) {
        const hipblasLtEpilogue_t epi = HIPBLASLT_EPILOGUE_BIAS;
        const int32_t bias_type = static_cast<int32_t>(dt);
        if (hipblasLtMatmulDescSetAttribute(p->desc, HIPBLASLT_MATMUL_DESC_EPILOGUE, &epi, sizeof(epi)) != HIPBLAS_STATUS_SUCCESS ||
            hipblasLtMatmulDescSetAttribute(p->desc, HIPBLASLT_MATMUL_DESC_BIAS_DATA_TYPE, &bias_type, sizeof(bias_type)) !=
                HIPBLAS_STATUS_SUCCESS)
            return p;
    }
    if (hipblasLtMatrixLayoutCreate(&p->a, dt, uint64_t(key.K), uint64_t(key.M), key.K) != HIPBLAS_STATUS_SUCCESS ||
        hipblasLtMatrixLayoutCreate(&p->b, dt, uint64_t(key.K), uint64_t(key.rows), key.K) != HIPBLAS_STATUS_SUCCESS ||
        hipblasLtMatrixLayoutCreate(&p->c, dt, uint64_t(key.M), uint64_t(key.rows), key.M) != HIPBLAS_STATUS_SUCCESS)
        return p;
    hipblasLtMatmulPreference_t pref = nullptr;
    if (hipblasLtMatmulPreferenceCreate(&pref) != HIPBLAS_STATUS_SUCCESS) return p;
    const uint64_t max_ws = kLtMaxWorkspace;
    hipblasLtMatmulHeuristicResult_t result{};
    int found = 0;
    if (hipblasLtMatmulPreferenceSetAttribute(pref, HIPBLASLT_MATMUL_PREF_MAX_WORKSPACE_BYTES, &max_ws, sizeof(max_ws)) == HIPBLAS_STATUS_SUCCESS &&
        hipblasLtMatmulAlgoGetHeuristic(handle, p->desc, p->a, p->b, p->c, p->c, pref, 1, &result, &found) == HIPBLAS_STATUS_SUCCESS &&
        found > 0 && result.state == HIPBLAS_STATUS_SUCCESS && result.workspaceSize <= kLtMaxWorkspace) {
        p->algo = result.algo;
        p->workspace = result.workspaceSize;
        p->usable = true;
    }
    hipblasLtMatmulPreferenceDestroy(pref);
    return p;
}

// out [.., M] = x [.., K] @ weight[M, K]^T (+ bias) through the cached hipBLASLt plan; false = not covered (the caller uses at::linear)
bool lt_linear(const torch::Tensor &x, const torch::Tensor &weight, const c10::optional<torch::Tensor> &bias, torch::Tensor &out) {
    hipDataType dt;
    switch (x.scalar_type()) {
        case torch::kBFloat16: dt = HIP_R_16BF; break;
        case torch::kFloat16: dt = HIP_R_16F; break;
        case torch::kFloat32: dt = HIP_R_32F; break;
        default: return false;
    }
    const int64_t K = weight.size(1), M = weight.size(0);
    if (x.dim() < 1 || x.size(-1) != K || !x.is_cuda() || x.device() != weight.device() || weight.scalar_type() != x.scalar_type() ||
        K <= 0 || M <= 0)
        return false;
    const int64_t rows = x.numel() / K;
    if (rows <= 0 || rows > (int64_t(1) << 30)) return false;
    if (bias.has_value() && (!bias->is_cuda() || bias->device() != x.device() || bias->scalar_type() != x.scalar_type() ||
                             bias->numel() != M || !bias->is_contiguous()))
        return false;
    const int device = x.device().index();
    hipStream_t stream = c10::hip::getCurrentHIPStream(device).stream();
    hipblasLtHandle_t handle = lt_handle(device, false);
    if (!handle) {  // first GEMM on this device: creating the library handle is not permitted under stream capture - hand the call to
                    // at::linear, which (measured) fails there exactly as a dense torch GEMM does: warm up before capturing, as always
        hipStreamCaptureStatus capturing = hipStreamCaptureStatusNone;
        (void)hipStreamIsCapturing(stream, &capturing);
        if (capturing != hipStreamCaptureStatusNone) return false;
        handle = lt_handle(device, true);
        if (!handle) return false;
    }
    LtPlan *plan = lt_plan(handle, LtKey{device, int(dt), bias.has_value() ? 1 : 0, rows, M, K}, dt);
    if (!plan->usable) return false;
    const torch::Tensor xc = x.is_contiguous() ? x : x.contiguous();
    auto shape = x.sizes().vec();
    shape.back() = M;
    out = torch::empty(shape, x.options());
    torch::Tensor ws;
    void *ws_ptr = nullptr;
    if (plan->workspace > 0) {  // from torch's caching allocator: stream-ordered, no synchronisation, fine under graph capture
        ws = torch::empty({int64_t(plan->workspace)}, x.options().dtype(torch::kUInt8));
        ws_ptr = ws.data_ptr();
    }
    if (bias.has_value()) {
        const void *bp = bias->data_ptr();
        if (hipblasLtMatmulDescSetAttribute(plan->desc, HIPBLASLT_MATMUL_DESC_BIAS_POINTER, &bp, sizeof(bp)) != HIPBLAS_STATUS_SUCCESS) return false;
    }
    const float alpha = 1.0f, beta = 0.0f;
    const hipblasStatus_t st = hipblasLtMatmul(handle, plan->desc, &alpha, weight.data_ptr(), plan->a, xc.data_ptr(), plan->b, &beta,
                                               out.data_ptr(), plan->c, out.data_ptr(), plan->c, &plan->algo, ws_ptr, plan->workspace, stream);
    if (st != HIPBLAS_STATUS_SUCCESS) {
        plan->usable = false;  // do not try this shape again
        return false;
    }
    return true;
}

torch::Tensor qlinear_impl(const torch::Tensor &A_in, const torch::Tensor &A, const torch::Tensor &absmax, int M, int N,
                           int blocksize, int table, const c10::optional<torch::Tensor> &bias) {
    check_gpu_contiguous(A, "A");
    check_gpu_contiguous(absmax, "absmax");
    torch::Tensor weight = torch::empty({M, N}, A_in.options());
    // the GEMM below reads the weight straight back: keep it in L2 / Infinity Cache (plain stores)
    dequant_into(A, absmax, weight, blocksize, int64_t(M) * N, table, FP4_DEQUANT_KEEP_CACHED);
    // at::linear is more than a product under autograd (gradient to the activation and the bias) and under autocast (its cast policy)
    const bool wants_grad = at::GradMode::is_enabled() && (A_in.requires_grad() || (bias.has_value() && bias->requires_grad()));
    if (qlinear_gemm_direct() && !wants_grad && !at::autocast::is_autocast_enabled(A_in.device().type())) {
        c10::DeviceGuard guard(A_in.device());
        torch::Tensor out;
        if (lt_linear(A_in, weight, bias, out)) {
            g_qlinear_direct_calls.fetch_add(1, std::memory_order_relaxed);
            return out;
        }
    }
    g_qlinear_aten_calls.fetch_add(1, std::memory_order_relaxed);
    return bias.has_value() ? at::linear(A_in, weight, *bias) : at::linear(A_in, weight);
}

torch::Tensor qlinear(torch::Tensor A_in, torch::Tensor A, torch::Tensor absmax, int M, int N, int blocksize) {
    return qlinear_impl(A_in, A, absmax, M, N, blocksize, FP4_TABLE_TREE, c10::nullopt);
}
torch::Tensor qlinear_bias(torch::Tensor A_in, torch::Tensor A, torch::Tensor absmax, int M, int N, int blocksize,
                           torch::Tensor bias) {
    return qlinear_impl(A_in, A, absmax, M, N, blocksize, FP4_TABLE_TREE, bias);
}
torch::Tensor qlinear_codebook(torch::Tensor A_in, torch::Tensor A, torch::Tensor absmax, torch::Tensor codebook, int M, int N,
                               int blocksize) {
    return qlinear_impl(A_in, A, absmax, M, N, blocksize, FP4_TABLE_CODEBOOK, c10::nullopt);
}
torch::Tensor qlinear_codebook_bias(torch::Tensor A_in, torch::Tensor A, torch::Tensor absmax, torch::Tensor codebook, int M,
                                    int N, int blocksize, torch::Tensor bias) {
    return qlinear_impl(A_in, A, absmax, M, N, blocksize, FP4_TABLE_CODEBOOK, bias);
}

torch::Tensor qlinear_nf4(torch::Tensor A_in, torch::Tensor A, torch::Tensor absmax, int M, int N, int blocksize) {
    return qlinear_impl(A_in, A, absmax, M, N, blocksize, FP4_TABLE_NF4, c10::nullopt);
}
torch::Tensor qlinear_nf4_bias(torch::Tensor A_in, torch::Tensor A, torch::Tensor absmax, int M, int N, int blocksize, torch::Tensor bias) {
    return qlinear_impl(A_in, A, absmax, M, N, blocksize, FP4_TABLE_NF4, bias);
}

// datatype == nullptr: the NF4 GEMV (its code is fixed; the FP4 ops take the reference's `datatype` tensor and ignore it)
torch::Tensor gemv_impl(const torch::Tensor &A, const torch::Tensor &B, const torch::Tensor &absmax,
                        const torch::Tensor *datatype, int blocksize, ScalarTypeEnum dtype, const std::vector<uint32_t> &Bshape,
                        const c10::optional<torch::Tensor> &bias) {
    check_gpu_contiguous(A, "A");
    check_gpu_contiguous(B, "B");
    check_gpu_contiguous(absmax, "absmax");
    if (datatype) check_gpu_contiguous(*datatype, "datatype");
    const char *op = datatype ? "gemv_fp4" : "gemv_nf4";
    TORCH_CHECK(Bshape.size() == 2, "Bshape must be the [out_features, in_features] of the quantised weight");
    const int64_t m = Bshape[0], k = Bshape[1];
    const torch::ScalarType st = to_torch(dtype);
    // reference: per-dtype TORCH_CHECKs of csrc/gemv_fp4_optimized.cu:303-305,323-325,343-345
    TORCH_CHECK(A.scalar_type() == st, op, ": dtype argument (", st, ") must equal the activation dtype (", A.scalar_type(), ")");
    TORCH_CHECK(absmax.scalar_type() == torch::kFloat32, "Only fp32 absmax is supported");
    TORCH_CHECK(!datatype || datatype->scalar_type() == torch::kFloat32, "Only fp32 code is supported");
    TORCH_CHECK(B.dtype() == torch::kUInt8, "B must be uint8");
    TORCH_CHECK(A.dim() == 2 || A.dim() == 3, op, ": activation must be [1, K] or [1, 1, K]");
    TORCH_CHECK(A.numel() == k && A.size(-1) == k, op, " is batch-1 only: activation has ", A.numel(),
                " elements, in_features is ", k);
    TORCH_CHECK(B.numel() * 2 >= m * k, "B holds ", B.numel(), " bytes, ", m * k / 2, " needed");
    TORCH_CHECK(absmax.numel() * int64_t(blocksize) >= m * k, "absmax too small for a ", m, "x", k, " weight");
    TORCH_CHECK(B.device() == A.device() && absmax.device() == A.device(), "all tensors must be on one device");
    // reference output shape: [A.size(0), m] or [A.size(0), A.size(1), m] (csrc/gemv_fp4_optimized.cu:296-299)
    torch::Tensor out = A.dim() == 3 ? torch::empty({A.size(0), A.size(1), m}, A.options()) : torch::empty({A.size(0), m}, A.options());
    torch::Tensor bias_c;
    const void *bias_ptr = epilogue_operand(op, "bias", bias, m, st, A.device(), bias_c);
    c10::DeviceGuard guard(A.device());
    const auto gemv = datatype ? fp4_hip_gemv : fp4_hip_gemv_nf4;
    check_status(gemv(A.data_ptr(), B.data_ptr<uint8_t>(), absmax.data_ptr<float>(), bias_ptr, out.data_ptr(), m, k, blocksize, (int)dtype,
                      current_stream(A)));
    return out;
}

torch::Tensor gemv_fp4(torch::Tensor A, torch::Tensor B, torch::Tensor absmax, torch::Tensor datatype, int blocksize,
                       ScalarTypeEnum dtype, std::vector<uint32_t> Bshape) {
    return gemv_impl(A, B, absmax, &datatype, blocksize, dtype, Bshape, c10::nullopt);
}
torch::Tensor gemv_fp4_bias(torch::Tensor A, torch::Tensor B, torch::Tensor absmax, torch::Tensor datatype, int blocksize,
                            ScalarTypeEnum dtype, std::vector<uint32_t> Bshape, torch::Tensor bias) {
    return gemv_impl(A, B, absmax, &datatype, blocksize, dtype, Bshape, bias);
}
torch::Tensor gemv_nf4(torch::Tensor A, torch::Tensor B, torch::Tensor absmax, int blocksize, ScalarTypeEnum dtype,
                       std::vector<uint32_t> Bshape) {
    return gemv_impl(A, B, absmax, nullptr, blocksize, dtype, Bshape, c10::nullopt);
}
torch::Tensor gemv_nf4_bias(torch::Tensor A, torch::Tensor B, torch::Tensor absmax, int blocksize, ScalarTypeEnum dtype,
                            std::vector<uint32_t> Bshape, torch::Tensor bias) {
    return gemv_impl(A, B, absmax, nullptr, blocksize, dtype, Bshape, bias);
}

// ---- the fused 4-bit weight ops: one validated preamble ----------------------------------------------------------------------------
// Each op below takes an activation A [.., k], the packed weight B (uint8, two codes a byte), its float32 absmax (one scale per
// `blocksize` weights) and Bshape = [m, k], optionally a bias [m] and a residual of the output's shape, and returns a fresh tensor:
// A's shape with the last dimension replaced by m - or by m / 2 under the gated epilogue, silu(gate) * up over a weight whose rows
// interleave a gate and an up projection.  weight_op() is the only place they validate and allocate; an op is then that call, the
// device guard and the C ABI call it stands for.  One torch allocation (the output), no sync: every op can be captured in a graph.
struct WeightOp {
    const char *name;
    int64_t max_rows;      // the op covers 1..max_rows activation rows; 1: a batch-1 GEMV
    bool f32_out = false;  // the output is float32 [1, m] (gemv_fp4_partial), not of the activation's dtype and shape
};

struct WeightCall {
    int64_t m, k, rows, m_out;
    int dt;                            // FP4_DTYPE_* of the activation
    torch::Tensor out, bias_c, res_c;  // bias_c / res_c own what bias_ptr / res_ptr point to
    const void *bias_ptr, *res_ptr;
};

// absmax == nullptr: the op reads its scales from elsewhere (gemv_nf4_nested: check_nested)
WeightCall weight_op(const WeightOp &op, const torch::Tensor &A, const torch::Tensor &B, const torch::Tensor *absmax, int blocksize,
                     const std::vector<uint32_t> &Bshape, const c10::optional<torch::Tensor> &bias,
                     const c10::optional<torch::Tensor> &residual, int epilogue) {
    check_gpu_contiguous(A, "A", op.name);
    check_gpu_contiguous(B, "B", op.name);
    if (absmax) check_gpu_contiguous(*absmax, "absmax", op.name);
    TORCH_CHECK(Bshape.size() == 2, op.name, ": Bshape must be the [out_features, in_features] of the quantised weight");
    WeightCall w;
    const int64_t m = w.m = Bshape[0], k = w.k = Bshape[1];
    TORCH_CHECK(epilogue == FP4_EPILOGUE_NONE || epilogue == FP4_EPILOGUE_SILU_MUL_PAIRS, op.name, ": unknown epilogue ", epilogue);
    w.m_out = epilogue == FP4_EPILOGUE_SILU_MUL_PAIRS ? m / 2 : m;
    if (op.max_rows == 1) {
        TORCH_CHECK(A.dim() >= 1 && k > 0 && A.size(-1) == k && A.numel() == k, op.name, " is batch-1 only: activation has ", A.numel(),
                    " elements, in_features is ", k);
        w.rows = 1;
    } else {
        TORCH_CHECK(A.dim() >= 1 && k > 0 && A.size(-1) == k, op.name, ": last dim of the activation must be in_features = ", k);
        w.rows = A.numel() / k;
        TORCH_CHECK(w.rows >= 1 && w.rows <= op.max_rows, op.name, " covers 1..", op.max_rows, " activation rows, got ", w.rows);
    }
    TORCH_CHECK(B.scalar_type() == torch::kUInt8 && B.numel() * 2 >= m * k, op.name, ": B must be uint8, ", (m * k + 1) / 2,
                " bytes for a ", m, "x", k, " weight; B holds ", B.numel(), " of ", B.scalar_type(), ": too small");
    if (absmax)
        TORCH_CHECK(absmax->scalar_type() == torch::kFloat32 && absmax->numel() * int64_t(blocksize) >= m * k, op.name,
                    ": Only fp32 absmax is supported, one scale per ", blocksize, " weights of a ", m, "x", k, " weight; absmax holds ",
                    absmax->numel(), " of ", absmax->scalar_type(), ": absmax too small");
    check_on_device(op.name, "B", B, A);
    if (absmax) check_on_device(op.name, "absmax", *absmax, A);
    w.dt = to_fp4_dtype(A.scalar_type(), op.name);
    if (op.f32_out) {
        w.out = torch::empty({1, m}, A.options().dtype(torch::kFloat32));
    } else {
        auto shape = A.sizes().vec();
        shape.back() = w.m_out;
        w.out = torch::empty(shape, A.options());
    }
    w.bias_ptr = epilogue_operand(op.name, "bias", bias, m, A.scalar_type(), A.device(), w.bias_c);
    w.res_ptr = epilogue_operand(op.name, "residual", residual, w.rows * w.m_out, A.scalar_type(), A.device(), w.res_c);
    return w;
}

// GEMV with a fused epilogue (fp4_hip_gemv_fused): bias, residual add, silu(gate) * up.  A is [1, K] / [1, 1, K].
torch::Tensor gemv_fp4_fused(torch::Tensor A, torch::Tensor B, torch::Tensor absmax, int blocksize, std::vector<uint32_t> Bshape,
                             c10::optional<torch::Tensor> bias, c10::optional<torch::Tensor> residual, int epilogue) {
    WeightCall w = weight_op({"gemv_fp4_fused", 1}, A, B, &absmax, blocksize, Bshape, bias, residual, epilogue);
    c10::DeviceGuard guard(A.device());
    check_status(fp4_hip_gemv_fused(A.data_ptr(), B.data_ptr<uint8_t>(), absmax.data_ptr<float>(), w.bias_ptr, w.res_ptr, w.out.data_ptr(),
                                    w.m, w.k, blocksize, w.dt, epilogue, current_stream(A)));
    return std::move(w.out);
}

// Short weight x long rows: the split-K path of the FP4 small-batch product wants a scratch buffer (a second allocation, from torch's
// caching allocator: no sync, graph-capturable).  True if the library asked for one and the call was made through it.
bool gemm_small_fp4_with_workspace(const WeightCall &w, const torch::Tensor &A, const torch::Tensor &B, const torch::Tensor &absmax,
                                   int blocksize, int epilogue) {
    const int64_t ws_bytes = fp4_hip_gemm_small_ws_bytes(w.rows, w.m, w.k, blocksize, w.dt);
    if (ws_bytes <= 0) return false;
    torch::Tensor ws = torch::empty({ws_bytes}, A.options().dtype(torch::kUInt8));
    check_status(fp4_hip_gemm_small_ws(A.data_ptr(), B.data_ptr<uint8_t>(), absmax.data_ptr<float>(), w.bias_ptr, w.res_ptr, w.out.data_ptr(),
                                       w.rows, w.m, w.k, blocksize, w.dt, epilogue, ws.data_ptr(), ws_bytes, current_stream(A)));
    return true;
}

// fused small-batch product (fp4_hip_gemm_small): A [..., K] with 1..128 rows in total; raises if the shape is not covered
torch::Tensor gemm_small_fp4(torch::Tensor A, torch::Tensor B, torch::Tensor absmax, int blocksize, std::vector<uint32_t> Bshape,
                             c10::optional<torch::Tensor> bias) {
    WeightCall w = weight_op({"gemm_small_fp4", 128}, A, B, &absmax, blocksize, Bshape, bias, c10::nullopt, FP4_EPILOGUE_NONE);
    c10::DeviceGuard guard(A.device());
    if (!gemm_small_fp4_with_workspace(w, A, B, absmax, blocksize, FP4_EPILOGUE_NONE))
        check_status(fp4_hip_gemm_small(A.data_ptr(), B.data_ptr<uint8_t>(), absmax.data_ptr<float>(), w.bias_ptr, w.out.data_ptr(), w.rows,
                                        w.m, w.k, blocksize, w.dt, current_stream(A)));
    return std::move(w.out);
}

// the small-batch product with the fused epilogues (fp4_hip_gemm_small_fused)
torch::Tensor gemm_small_fp4_fused(torch::Tensor A, torch::Tensor B, torch::Tensor absmax, int blocksize, std::vector<uint32_t> Bshape,
                                   c10::optional<torch::Tensor> bias, c10::optional<torch::Tensor> residual, int epilogue) {
    WeightCall w = weight_op({"gemm_small_fp4_fused", 128}, A, B, &absmax, blocksize, Bshape, bias, residual, epilogue);
    c10::DeviceGuard guard(A.device());
    if (!gemm_small_fp4_with_workspace(w, A, B, absmax, blocksize, epilogue))
        check_status(fp4_hip_gemm_small_fused(A.data_ptr(), B.data_ptr<uint8_t>(), absmax.data_ptr<float>(), w.bias_ptr, w.res_ptr,
                                              w.out.data_ptr(), w.rows, w.m, w.k, blocksize, w.dt, epilogue, current_stream(A)));
    return std::move(w.out);
}

// fused NF4 products on the matrix cores; raise if the shape is not covered (blocksize 64, fp16 / bf16).  gemm_small_nf4
// (fp4_hip_gemm_small_nf4): 1..16 rows, K % 512 == 0.  gemm_wide_nf4 (fp4_hip_gemm_wide_nf4): 1..128 rows, K % 64 == 0.
torch::Tensor gemm_nf4_impl(const WeightOp &op, decltype(&fp4_hip_gemm_small_nf4) entry, const torch::Tensor &A, const torch::Tensor &B,
                            const torch::Tensor &absmax, int blocksize, const std::vector<uint32_t> &Bshape,
                            const c10::optional<torch::Tensor> &bias) {
    WeightCall w = weight_op(op, A, B, &absmax, blocksize, Bshape, bias, c10::nullopt, FP4_EPILOGUE_NONE);
    c10::DeviceGuard guard(A.device());
    check_status(entry(A.data_ptr(), B.data_ptr<uint8_t>(), absmax.data_ptr<float>(), w.bias_ptr, w.out.data_ptr(), w.rows, w.m, w.k,
                       blocksize, w.dt, current_stream(A)));
    return std::move(w.out);
}
torch::Tensor gemm_small_nf4(torch::Tensor A, torch::Tensor B, torch::Tensor absmax, int blocksize, std::vector<uint32_t> Bshape,
                             c10::optional<torch::Tensor> bias) {
    return gemm_nf4_impl({"gemm_small_nf4", 16}, fp4_hip_gemm_small_nf4, A, B, absmax, blocksize, Bshape, bias);
}
torch::Tensor gemm_wide_nf4(torch::Tensor A, torch::Tensor B, torch::Tensor absmax, int blocksize, std::vector<uint32_t> Bshape,
                            c10::optional<torch::Tensor> bias) {
    return gemm_nf4_impl({"gemm_wide_nf4", 128}, fp4_hip_gemm_wide_nf4, A, B, absmax, blocksize, Bshape, bias);
}

// the operands of the LoRA forms: lora_B [m, R] of the activation dtype over the weight's rows - with `stack` B_stack [n_adapters, m, R] -
// and t [rows, R] float32 (lora_down's output, with `stack` lora_down_multi's); -> R
int64_t check_lora(const char *op, const torch::Tensor &A, const WeightCall &w, const torch::Tensor &lora_B, const torch::Tensor &t,
                   bool stack = false) {
    const char *name = stack ? "B_stack" : "lora_B";
    const int64_t lead = stack ? 1 : 0;  // the dimensions ahead of [m, R]
    check_gpu_contiguous(lora_B, name, op);
    check_gpu_contiguous(t, "t", op);
    TORCH_CHECK(lora_B.dim() == 2 + lead && (!stack || lora_B.size(0) >= 1) && lora_B.size(lead) == w.m &&
                    lora_B.scalar_type() == A.scalar_type() && lora_B.device() == A.device(),
                op, ": ", name, " must be a [", stack ? "n_adapters, " : "", w.m, ", R] tensor of the activation dtype on the activation's device");
    const int64_t R = lora_B.size(lead + 1);
    TORCH_CHECK(t.scalar_type() == torch::kFloat32 && t.numel() == w.rows * R && t.device() == A.device(), op, ": t must hold ", w.rows * R,
                " float32 elements (", stack ? "lora_down_multi" : "lora_down", "'s output) on the activation's device");
    return R;
}

// LoRA adapters beside an NF4 weight.  lora_down: t = scale * (x @ A^T) as float32 [rows, R] (fp4_hip_lora_down; x [.., K] with
// 1..64 rows, A [R, K] of x's dtype, scale float32 [R]).  gemv_nf4_lora / gemm_nf4_lora: gemv_nf4_fused / gemm_nf4_fused with
// lora_B @ t added to the f32 row sums before the rounding (fp4_hip_gemv_lora_nf4 / fp4_hip_gemm_lora_nf4).  One allocation each.
torch::Tensor lora_down(torch::Tensor x, torch::Tensor A, torch::Tensor scale) {
    check_gpu_contiguous(x, "x");
    check_gpu_contiguous(A, "A");
    check_gpu_contiguous(scale, "scale");
    TORCH_CHECK(A.dim() == 2, "lora_down: A must be [R, in_features]");
    const int64_t R = A.size(0), k = A.size(1);
    TORCH_CHECK(x.dim() >= 1 && k > 0 && x.size(-1) == k, "lora_down: last dim of the activation must be in_features = ", k);
    TORCH_CHECK(A.scalar_type() == x.scalar_type(), "lora_down: A must have the activation's dtype");
    TORCH_CHECK(scale.scalar_type() == torch::kFloat32 && scale.numel() == R, "lora_down: scale must hold ", R, " float32 factors");
    TORCH_CHECK(A.device() == x.device() && scale.device() == x.device(), "all tensors must be on one device");
    const int64_t rows = x.numel() / k;
    const int dt = to_fp4_dtype(x.scalar_type(), "lora_down");
    torch::Tensor t = torch::empty({rows, R}, x.options().dtype(torch::kFloat32));
    c10::DeviceGuard guard(x.device());
    check_status(fp4_hip_lora_down(x.data_ptr(), A.data_ptr(), scale.data_ptr<float>(), t.data_ptr<float>(), rows, R, k, dt, current_stream(x)));
    return t;
}
// Several adapters in one batch, selected per activation row on the device.  ids: int32, contiguous, on the activation's device, at
// least `rows` elements (the first `rows` are used; it is never read on the host, so a captured step follows an in-place rewrite).
void check_ids(const char *op, const torch::Tensor &ids, const torch::Tensor &x, int64_t rows) {
    check_gpu_contiguous(ids, "ids", op);
    TORCH_CHECK(ids.scalar_type() == torch::kInt32 && ids.device() == x.device() && ids.numel() >= rows, op, ": ids must be a contiguous int32 "
                "tensor on the activation's device with at least one element per activation row (", rows, ")");
}
// lora_down_multi: t[b] = scale_stack[ids[b]] * (x[b] @ A_stack[ids[b]]^T), +0 where ids[b] names no adapter (fp4_hip_lora_down_multi;
// A_stack [n, R, K] of x's dtype, scale_stack float32 [n, R]).
torch::Tensor lora_down_multi(torch::Tensor x, torch::Tensor A_stack, torch::Tensor scale_stack, torch::Tensor ids) {
    const char *op = "lora_down_multi";
    check_gpu_contiguous(x, "x", op);
    check_gpu_contiguous(A_stack, "A_stack", op);
    check_gpu_contiguous(scale_stack, "scale_stack", op);
    TORCH_CHECK(A_stack.dim() == 3 && A_stack.size(0) >= 1, op, ": A_stack must be [n_adapters, R, in_features] with at least one adapter");
    const int64_t n = A_stack.size(0), R = A_stack.size(1), k = A_stack.size(2);
    TORCH_CHECK(x.dim() >= 1 && k > 0 && x.size(-1) == k, op, ": last dim of the activation must be in_features = ", k);
    TORCH_CHECK(A_stack.scalar_type() == x.scalar_type(), op, ": A_stack must have the activation's dtype");
    TORCH_CHECK(scale_stack.scalar_type() == torch::kFloat32 && scale_stack.dim() == 2 && scale_stack.size(0) == n && scale_stack.size(1) == R,
                op, ": scale_stack must be a float32 [", n, ", ", R, "] tensor");
    TORCH_CHECK(A_stack.device() == x.device() && scale_stack.device() == x.device(), op, ": all tensors must be on one device");
    const int64_t rows = x.numel() / k;
    check_ids(op, ids, x, rows);
    const int dt = to_fp4_dtype(x.scalar_type(), op);
    torch::Tensor t = torch::empty({rows, R}, x.options().dtype(torch::kFloat32));
    c10::DeviceGuard guard(x.device());
    check_status(fp4_hip_lora_down_multi(x.data_ptr(), A_stack.data_ptr(), scale_stack.data_ptr<float>(), ids.data_ptr<int32_t>(),
                                         t.data_ptr<float>(), rows, n, R, k, dt, current_stream(x)));
    return t;
}
// ---- nested (double-quantised) absmax: bitsandbytes' compress_statistics ------------------------------------------------------------
// absmax_u8 uint8 [nb], nested_absmax float32 [ceil(nb / nested_blocksize)], code float32 [256], offset a Python float (passed to the
// kernel by value: no device read of a host scalar, no sync).
void check_nested(const char *op, const torch::Tensor &absmax_u8, const torch::Tensor &nested_absmax, const torch::Tensor &code,
                  int64_t nested_blocksize, int64_t nb) {
    check_gpu_contiguous(absmax_u8, "absmax_u8");
    check_gpu_contiguous(nested_absmax, "nested_absmax");
    check_gpu_contiguous(code, "nested_code");
    TORCH_CHECK(absmax_u8.scalar_type() == torch::kUInt8, op, ": absmax_u8 must be uint8");
    TORCH_CHECK(nested_absmax.scalar_type() == torch::kFloat32 && code.scalar_type() == torch::kFloat32, op,
                ": nested_absmax and nested_code must be float32");
    TORCH_CHECK(code.numel() == 256, op, ": nested_code must hold 256 entries, got ", code.numel());
    TORCH_CHECK(nested_blocksize > 0, op, ": nested_blocksize must be positive");
    TORCH_CHECK(absmax_u8.numel() >= nb, op, ": absmax_u8 holds ", absmax_u8.numel(), " codes, ", nb, " needed");
    TORCH_CHECK(nested_absmax.numel() >= (nb + nested_blocksize - 1) / nested_blocksize, op, ": nested_absmax holds ", nested_absmax.numel(),
                " group scales, ", (nb + nested_blocksize - 1) / nested_blocksize, " needed");
    TORCH_CHECK(nested_absmax.device() == absmax_u8.device() && code.device() == absmax_u8.device(), op, ": all tensors must be on one device");
}

torch::Tensor absmax_unnest(torch::Tensor absmax_u8, torch::Tensor nested_absmax, torch::Tensor code, double offset, int64_t nested_blocksize) {
    const int64_t nb = absmax_u8.numel();
    check_nested("absmax_unnest", absmax_u8, nested_absmax, code, nested_blocksize, nb);
    torch::Tensor out = torch::empty({nb}, absmax_u8.options().dtype(torch::kFloat32));
    c10::DeviceGuard guard(absmax_u8.device());
    check_status(fp4_hip_absmax_unnest(absmax_u8.data_ptr<uint8_t>(), nested_absmax.data_ptr<float>(), code.data_ptr<float>(), (float)offset,
                                       (int)nested_blocksize, nb, out.data_ptr<float>(), current_stream(absmax_u8)));
    return out;
}

// (absmax float32 [nb], offset, code float32 [256], nested_blocksize) -> (absmax_u8 uint8 [nb], nested_absmax float32 [ceil(nb / g)])
std::tuple<torch::Tensor, torch::Tensor> absmax_nest(torch::Tensor absmax, double offset, torch::Tensor code, int64_t nested_blocksize) {
    check_gpu_contiguous(absmax, "absmax");
    check_gpu_contiguous(code, "nested_code");
    TORCH_CHECK(absmax.scalar_type() == torch::kFloat32 && code.scalar_type() == torch::kFloat32, "absmax_nest: absmax and nested_code must be float32");
    TORCH_CHECK(code.numel() == 256 && code.device() == absmax.device(), "absmax_nest: nested_code must hold 256 entries on absmax's device");
    TORCH_CHECK(nested_blocksize > 0, "absmax_nest: nested_blocksize must be positive");
    const int64_t nb = absmax.numel();
    torch::Tensor q = torch::empty({nb}, absmax.options().dtype(torch::kUInt8));
    torch::Tensor nested = torch::empty({(nb + nested_blocksize - 1) / nested_blocksize}, absmax.options());
    c10::DeviceGuard guard(absmax.device());
    check_status(fp4_hip_absmax_nest(absmax.data_ptr<float>(), nb, (float)offset, code.data_ptr<float>(), (int)nested_blocksize,
                                     q.data_ptr<uint8_t>(), nested.data_ptr<float>(), current_stream(absmax)));
    return {q, nested};
}

// ---- the NF4 decode ops: one wrapper for the ten C entry points -----------------------------------------------------------------------
// gemv_nf4_fused / gemm_nf4_fused are the NF4 twins of gemv_fp4_fused / gemm_small_fp4_fused (fp4_hip_gemv_fused_nf4 / fp4_hip_gemm_fused_nf4).
// An op may add ONE of: an adapter (*_lora: lora_B @ t added to the f32 row sums before the rounding) or a stack of adapters
// (*_lora_multi: B_stack [n, m, R], the adapter of row b read from ids[b] on the device; a row without one is the plain fused op's),
// and, without a stack, read the statistics compressed (*_nested, *_lora_nested: the un-nested op's shapes with absmax_u8,
// nested_absmax, code, offset, nested_blocksize in absmax's place).  One allocation each.
struct LoraOperands {
    const torch::Tensor &lora_B, &t;
};
struct StackOperands {
    const torch::Tensor &B_stack, &ids, &t;
};
struct NestedOperands {
    const torch::Tensor &absmax_u8, &nested_absmax, &code;
    double offset;
    int64_t nested_blocksize;
};

// absmax: the float32 scales, or nullptr with `nested`
torch::Tensor nf4_decode_op(const char *op, bool gemv, const torch::Tensor &A, const torch::Tensor &B, const torch::Tensor *absmax, int blocksize,
                            const std::vector<uint32_t> &Bshape, const c10::optional<torch::Tensor> &bias,
                            const c10::optional<torch::Tensor> &residual, int epilogue, const LoraOperands *adapter, const StackOperands *stack,
                            const NestedOperands *nested) {
    if (nested) TORCH_CHECK(blocksize > 0, op, ": blocksize must be positive");
    WeightCall w = weight_op({op, gemv ? 1 : 128}, A, B, absmax, blocksize, Bshape, bias, residual, epilogue);
    if (nested) {
        check_nested(op, nested->absmax_u8, nested->nested_absmax, nested->code, nested->nested_blocksize, (w.m * w.k + blocksize - 1) / blocksize);
        check_on_device(op, "absmax_u8", nested->absmax_u8, A);
    }
    int64_t R = 0;
    if (adapter) R = check_lora(op, A, w, adapter->lora_B, adapter->t);
    if (stack) {
        R = check_lora(op, A, w, stack->B_stack, stack->t, true);
        check_ids(op, stack->ids, A, w.rows);
    }
    c10::DeviceGuard guard(A.device());
    const void *x = A.data_ptr();
    const uint8_t *W = B.data_ptr<uint8_t>();
    void *out = w.out.data_ptr(), *s = current_stream(A);
    int rc;
    if (nested) {
        const uint8_t *q = nested->absmax_u8.data_ptr<uint8_t>();
        const float *group = nested->nested_absmax.data_ptr<float>(), *table = nested->code.data_ptr<float>(), offset = (float)nested->offset;
        const int g = (int)nested->nested_blocksize;
        if (!adapter)
            rc = gemv ? fp4_hip_gemv_nested_nf4(x, W, q, group, table, offset, g, w.bias_ptr, w.res_ptr, out, w.m, w.k, blocksize, w.dt, epilogue, s)
                      : fp4_hip_gemm_nested_nf4(x, W, q, group, table, offset, g, w.bias_ptr, w.res_ptr, out, w.rows, w.m, w.k, blocksize, w.dt,
                                                epilogue, s);
        else
            rc = gemv ? fp4_hip_gemv_lora_nested_nf4(x, W, q, group, table, offset, g, w.bias_ptr, w.res_ptr, adapter->lora_B.data_ptr(),
                                                     adapter->t.data_ptr<float>(), R, out, w.m, w.k, blocksize, w.dt, epilogue, s)
                      : fp4_hip_gemm_lora_nested_nf4(x, W, q, group, table, offset, g, w.bias_ptr, w.res_ptr, adapter->lora_B.data_ptr(),
                                                     adapter->t.data_ptr<float>(), R, out, w.rows, w.m, w.k, blocksize, w.dt, epilogue, s);
    } else {
        const float *am = absmax->data_ptr<float>();
        if (stack) {
            const void *Bs = stack->B_stack.data_ptr();
            const int32_t *ids = stack->ids.data_ptr<int32_t>();
            const int64_t n = stack->B_stack.size(0);
            const float *t = stack->t.data_ptr<float>();
            rc = gemv ? fp4_hip_gemv_lora_multi_nf4(x, W, am, w.bias_ptr, w.res_ptr, Bs, ids, n, t, R, out, w.m, w.k, blocksize, w.dt, epilogue, s)
                      : fp4_hip_gemm_lora_multi_nf4(x, W, am, w.bias_ptr, w.res_ptr, Bs, ids, n, t, R, out, w.rows, w.m, w.k, blocksize, w.dt,
                                                    epilogue, s);
        } else if (adapter) {
            const void *lb = adapter->lora_B.data_ptr();
            const float *t = adapter->t.data_ptr<float>();
            rc = gemv ? fp4_hip_gemv_lora_nf4(x, W, am, w.bias_ptr, w.res_ptr, lb, t, R, out, w.m, w.k, blocksize, w.dt, epilogue, s)
                      : fp4_hip_gemm_lora_nf4(x, W, am, w.bias_ptr, w.res_ptr, lb, t, R, out, w.rows, w.m, w.k, blocksize, w.dt, epilogue, s);
        } else {
            rc = gemv ? fp4_hip_gemv_fused_nf4(x, W, am, w.bias_ptr, w.res_ptr, out, w.m, w.k, blocksize, w.dt, epilogue, s)
                      : fp4_hip_gemm_fused_nf4(x, W, am, w.bias_ptr, w.res_ptr, out, w.rows, w.m, w.k, blocksize, w.dt, epilogue, s);
        }
    }
    check_status(rc);
    return std::move(w.out);
}

torch::Tensor gemv_nf4_fused(torch::Tensor A, torch::Tensor B, torch::Tensor absmax, int blocksize, std::vector<uint32_t> Bshape,
                             c10::optional<torch::Tensor> bias, c10::optional<torch::Tensor> residual, int epilogue) {
    return nf4_decode_op("gemv_nf4_fused", true, A, B, &absmax, blocksize, Bshape, bias, residual, epilogue, nullptr, nullptr, nullptr);
}
torch::Tensor gemm_nf4_fused(torch::Tensor A, torch::Tensor B, torch::Tensor absmax, int blocksize, std::vector<uint32_t> Bshape,
                             c10::optional<torch::Tensor> bias, c10::optional<torch::Tensor> residual, int epilogue) {
    return nf4_decode_op("gemm_nf4_fused", false, A, B, &absmax, blocksize, Bshape, bias, residual, epilogue, nullptr, nullptr, nullptr);
}
torch::Tensor gemv_nf4_lora(torch::Tensor A, torch::Tensor B, torch::Tensor absmax, int blocksize, std::vector<uint32_t> Bshape,
                            c10::optional<torch::Tensor> bias, c10::optional<torch::Tensor> residual, int epilogue, torch::Tensor lora_B,
                            torch::Tensor t) {
    const LoraOperands adapter{lora_B, t};
    return nf4_decode_op("gemv_nf4_lora", true, A, B, &absmax, blocksize, Bshape, bias, residual, epilogue, &adapter, nullptr, nullptr);
}
torch::Tensor gemm_nf4_lora(torch::Tensor A, torch::Tensor B, torch::Tensor absmax, int blocksize, std::vector<uint32_t> Bshape,
                            c10::optional<torch::Tensor> bias, c10::optional<torch::Tensor> residual, int epilogue, torch::Tensor lora_B,
                            torch::Tensor t) {
    const LoraOperands adapter{lora_B, t};
    return nf4_decode_op("gemm_nf4_lora", false, A, B, &absmax, blocksize, Bshape, bias, residual, epilogue, &adapter, nullptr, nullptr);
}
torch::Tensor gemv_nf4_lora_multi(torch::Tensor A, torch::Tensor B, torch::Tensor absmax, int blocksize, std::vector<uint32_t> Bshape,
                                  c10::optional<torch::Tensor> bias, c10::optional<torch::Tensor> residual, int epilogue,
                                  torch::Tensor B_stack, torch::Tensor ids, torch::Tensor t) {
    const StackOperands stack{B_stack, ids, t};
    return nf4_decode_op("gemv_nf4_lora_multi", true, A, B, &absmax, blocksize, Bshape, bias, residual, epilogue, nullptr, &stack, nullptr);
}
torch::Tensor gemm_nf4_lora_multi(torch::Tensor A, torch::Tensor B, torch::Tensor absmax, int blocksize, std::vector<uint32_t> Bshape,
                                  c10::optional<torch::Tensor> bias, c10::optional<torch::Tensor> residual, int epilogue,
                                  torch::Tensor B_stack, torch::Tensor ids, torch::Tensor t) {
    const StackOperands stack{B_stack, ids, t};
    return nf4_decode_op("gemm_nf4_lora_multi", false, A, B, &absmax, blocksize, Bshape, bias, residual, epilogue, nullptr, &stack, nullptr);
}
torch::Tensor gemv_nf4_nested(torch::Tensor A, torch::Tensor B, torch::Tensor absmax_u8, torch::Tensor nested_absmax, torch::Tensor code,
                              double offset, int64_t nested_blocksize, int blocksize, std::vector<uint32_t> Bshape,
                              c10::optional<torch::Tensor> bias, c10::optional<torch::Tensor> residual, int epilogue) {
    const NestedOperands nested{absmax_u8, nested_absmax, code, offset, nested_blocksize};
    return nf4_decode_op("gemv_nf4_nested", true, A, B, nullptr, blocksize, Bshape, bias, residual, epilogue, nullptr, nullptr, &nested);
}
torch::Tensor gemm_nf4_nested(torch::Tensor A, torch::Tensor B, torch::Tensor absmax_u8, torch::Tensor nested_absmax, torch::Tensor code,
                              double offset, int64_t nested_blocksize, int blocksize, std::vector<uint32_t> Bshape,
                              c10::optional<torch::Tensor> bias, c10::optional<torch::Tensor> residual, int epilogue) {
    const NestedOperands nested{absmax_u8, nested_absmax, code, offset, nested_blocksize};
    return nf4_decode_op("gemm_nf4_nested", false, A, B, nullptr, blocksize, Bshape, bias, residual, epilogue, nullptr, nullptr, &nested);
}
torch::Tensor gemv_nf4_lora_nested(torch::Tensor A, torch::Tensor B, torch::Tensor absmax_u8, torch::Tensor nested_absmax, torch::Tensor code,
                                   double offset, int64_t nested_blocksize, int blocksize, std::vector<uint32_t> Bshape,
                                   c10::optional<torch::Tensor> bias, c10::optional<torch::Tensor> residual, int epilogue,
                                   torch::Tensor lora_B, torch::Tensor t) {
    const NestedOperands nested{absmax_u8, nested_absmax, code, offset, nested_blocksize};
    const LoraOperands adapter{lora_B, t};
    return nf4_decode_op("gemv_nf4_lora_nested", true, A, B, nullptr, blocksize, Bshape, bias, residual, epilogue, &adapter, nullptr, &nested);
}
torch::Tensor gemm_nf4_lora_nested(torch::Tensor A, torch::Tensor B, torch::Tensor absmax_u8, torch::Tensor nested_absmax, torch::Tensor code,
                                   double offset, int64_t nested_blocksize, int blocksize, std::vector<uint32_t> Bshape,
                                   c10::optional<torch::Tensor> bias, c10::optional<torch::Tensor> residual, int epilogue,
                                   torch::Tensor lora_B, torch::Tensor t) {
    const NestedOperands nested{absmax_u8, nested_absmax, code, offset, nested_blocksize};
    const LoraOperands adapter{lora_B, t};
    return nf4_decode_op("gemm_nf4_lora_nested", false, A, B, nullptr, blocksize, Bshape, bias, residual, epilogue, &adapter, nullptr, &nested);
}

// unnest into a temporary from the caching allocator (stream-ordered: no sync, capturable), then qlinear_nf4 / qlinear_nf4_bias
torch::Tensor qlinear_nf4_nested(torch::Tensor A_in, torch::Tensor A, torch::Tensor absmax_u8, torch::Tensor nested_absmax, torch::Tensor code,
                                 double offset, int64_t nested_blocksize, int M, int N, int blocksize, c10::optional<torch::Tensor> bias) {
    torch::Tensor absmax = absmax_unnest(absmax_u8, nested_absmax, code, offset, nested_blocksize);
    return qlinear_impl(A_in, A, absmax, M, N, blocksize, FP4_TABLE_NF4, bias);
}

// f32 partial sums of a K-split shard: [1, m] float32 (see fp4_hip_gemv_partial); Bshape is [out_features, in_features of this shard]
torch::Tensor gemv_fp4_partial(torch::Tensor A, torch::Tensor B, torch::Tensor absmax, int blocksize, std::vector<uint32_t> Bshape) {
    WeightCall w = weight_op({"gemv_fp4_partial", 1, true}, A, B, &absmax, blocksize, Bshape, c10::nullopt, c10::nullopt, FP4_EPILOGUE_NONE);
    c10::DeviceGuard guard(A.device());
    check_status(fp4_hip_gemv_partial(A.data_ptr(), B.data_ptr<uint8_t>(), absmax.data_ptr<float>(), w.out.data_ptr<float>(), w.m, w.k,
                                      blocksize, w.dt, current_stream(A)));
    return std::move(w.out);
}

// bitsandbytes-format FP4 / NF4 quantisation of a float tensor: returns (packed uint8[ceil(n/2), 1], absmax float32[ceil(n/bs)])
std::tuple<torch::Tensor, torch::Tensor> quantize_4bit(torch::Tensor W, int blocksize, bool nf4) {
    check_gpu_contiguous(W, "W");
    const int dt = to_fp4_dtype(W.scalar_type(), nf4 ? "quantize_nf4" : "quantize_fp4");
    const int64_t n = W.numel();
    TORCH_CHECK(blocksize > 0, "blocksize must be positive");
    torch::Tensor packed = torch::empty({(n + 1) / 2, 1}, torch::TensorOptions().dtype(torch::kUInt8).device(W.device()));
    torch::Tensor absmax = torch::empty({(n + blocksize - 1) / blocksize}, torch::TensorOptions().dtype(torch::kFloat32).device(W.device()));
    c10::DeviceGuard guard(W.device());
    const auto quantize = nf4 ? fp4_hip_quantize_blockwise_nf4 : fp4_hip_quantize_blockwise;
    check_status(quantize(W.data_ptr(), dt, packed.data_ptr<uint8_t>(), absmax.data_ptr<float>(), n, blocksize, current_stream(W)));
    return {packed, absmax};
}
std::tuple<torch::Tensor, torch::Tensor> quantize_fp4(torch::Tensor W, int blocksize) { return quantize_4bit(W, blocksize, false); }
std::tuple<torch::Tensor, torch::Tensor> quantize_nf4(torch::Tensor W, int blocksize) { return quantize_4bit(W, blocksize, true); }

// ---- one-shot all-reduce plumbing (fp4_hip_comm_* / fp4_hip_allreduce_oneshot) ---------------------------------------
// Buffers are identified by their device address (an int on the Python side); torch_bnb_fp4/comm.py owns their lifetime.
std::tuple<int64_t, py::bytes, int> comm_alloc(int world, int64_t capacity, int device) {
    const int64_t bytes = fp4_hip_comm_bytes(world, capacity);
    TORCH_CHECK(bytes > 0, "comm_alloc: bad world / capacity");
    c10::DeviceGuard guard(c10::Device(c10::kCUDA, (c10::DeviceIndex)device));
    void *p = nullptr;
    uint8_t handle[64];
    int kind = -1;
    check_status(fp4_hip_comm_alloc(bytes, &p, handle, &kind));
    return {reinterpret_cast<int64_t>(p), py::bytes(reinterpret_cast<const char *>(handle), 64), kind};
}

int64_t comm_open(const std::string &handle, int device) {
    TORCH_CHECK(handle.size() == 64, "comm_open: an IPC handle is 64 bytes");
    c10::DeviceGuard guard(c10::Device(c10::kCUDA, (c10::DeviceIndex)device));
    void *p = nullptr;
    check_status(fp4_hip_comm_open(reinterpret_cast<const uint8_t *>(handle.data()), &p));
    return reinterpret_cast<int64_t>(p);
}

void comm_close(int64_t ptr) { check_status(fp4_hip_comm_close(reinterpret_cast<void *>(ptr))); }
void comm_free(int64_t ptr) { check_status(fp4_hip_comm_free(reinterpret_cast<void *>(ptr))); }

std::vector<uint32_t> comm_status(int64_t own_ptr) {
    std::vector<uint32_t> out(4);
    check_status(fp4_hip_comm_status(reinterpret_cast<const void *>(own_ptr), out.data()));
    return out;
}

void comm_clear_status(int64_t own_ptr) { check_status(fp4_hip_comm_clear_status(reinterpret_cast<void *>(own_ptr))); }

// partial: f32 [.., M] on this rank's GPU; returns T [.., M] = T(sum over ranks) (+ bias) (+ residual)
torch::Tensor allreduce_oneshot(torch::Tensor partial, std::vector<int64_t> peers, int rank, int64_t capacity, ScalarTypeEnum dtype,
                                c10::optional<torch::Tensor> bias, c10::optional<torch::Tensor> residual, int64_t timeout_us) {
    check_gpu_contiguous(partial, "partial");
    TORCH_CHECK(partial.scalar_type() == torch::kFloat32, "allreduce_oneshot: the partial sums must be float32");
    const int world = (int)peers.size();
    const int64_t m = partial.numel();
    const torch::ScalarType st = to_torch(dtype);
    torch::Tensor out = torch::empty(partial.sizes(), partial.options().dtype(st));
    torch::Tensor bias_c, res_c;
    const void *bias_ptr = epilogue_operand("allreduce_oneshot", "bias", bias, m, st, partial.device(), bias_c);
    const void *res_ptr = epilogue_operand("allreduce_oneshot", "residual", residual, m, st, partial.device(), res_c);
    std::vector<void *> bufs(world);
    for (int p = 0; p < world; ++p) bufs[p] = reinterpret_cast<void *>(peers[p]);
    c10::DeviceGuard guard(partial.device());
    check_status(fp4_hip_allreduce_oneshot(partial.data_ptr<float>(), bufs.data(), rank, world, m, capacity, bias_ptr, res_ptr,
                                           out.data_ptr(), (int)dtype, timeout_us, current_stream(partial)));
    return out;
}

torch::Tensor code_table(const std::string &name) {
    TORCH_CHECK(name == "codebook" || name == "tree" || name == "nf4", "code_table: name must be 'codebook', 'tree' or 'nf4'");
    torch::Tensor t = torch::empty({16}, torch::kFloat32);
    const int table = name == "tree" ? FP4_TABLE_TREE : (name == "nf4" ? FP4_TABLE_NF4 : FP4_TABLE_CODEBOOK);
    check_status(fp4_hip_code_table(table, t.data_ptr<float>()));
    return t;
}

void set_kernel_variant(const std::string &kernel, int variant) { check_status(fp4_hip_set_variant(kernel.c_str(), variant)); }

}  // namespace

PYBIND11_MODULE(TORCH_EXTENSION_NAME, m) {
    m.doc() = "MI355X (gfx950) FP4 dequant / fused GEMV operators; same surface as aredden/torch-bnb-fp4's torch_bnb_fp4_ext";
    pybind11::enum_<ScalarTypeEnum>(m, "ScalarType")
        .value("bfloat16", ScalarTypeEnum::bfloat16)
        .value("float16", ScalarTypeEnum::float16)
        .value("float32", ScalarTypeEnum::float32)
        .export_values();

    m.def("dequantize_fp4", &dequantize_fp4, "FP4 -> T dequant, tree constants: (A, absmax, blocksize, M, N, o_type)");
    m.def("dequantize_fp4_codebook", &dequantize_fp4_codebook,
          "FP4 -> T dequant, CODE_PARAM table: (A, absmax, codebook, M, N, blocksize, n, dtype)");
    m.def("gemv_fp4", &gemv_fp4, "fused batch-1 FP4 GEMV: (A, B, absmax, datatype, blocksize, dtype, Bshape)");
    m.def("qlinear", &qlinear, "tree dequant + linear: (A_in, A, absmax, M, N, blocksize)");
    m.def("qlinear_bias", &qlinear_bias, "tree dequant + linear + bias");
    m.def("qlinear_codebook", &qlinear_codebook, "codebook dequant + linear: (A_in, A, absmax, codebook, M, N, blocksize)");
    m.def("qlinear_codebook_bias", &qlinear_codebook_bias, "codebook dequant + linear + bias");
    // extras
    m.def("gemv_fp4_bias", &gemv_fp4_bias, "gemv_fp4 with the bias add fused into the epilogue");
    m.def("gemv_fp4_fused", &gemv_fp4_fused,
          "GEMV with a fused epilogue: (A, B, absmax, blocksize, Bshape, bias|None, residual|None, epilogue) ; epilogue 0 = bias/residual, "
          "1 = silu(gate) * up over interleaved rows");
    m.def("gemm_small_fp4", &gemm_small_fp4, "fused FP4 product for 1..128 activation rows: (A, B, absmax, blocksize, Bshape, bias|None)");
    m.def("gemm_small_fp4_fused", &gemm_small_fp4_fused,
          "fused FP4 product for 1..128 rows with an epilogue: (A, B, absmax, blocksize, Bshape, bias|None, residual|None, epilogue)");
    m.def("gemv_fp4_partial", &gemv_fp4_partial, "f32 partial sums of a K-split shard: (A, B, absmax, blocksize, Bshape)");
    m.def("comm_alloc", &comm_alloc, "(world, capacity, device) -> (buffer address, 64-byte IPC handle, memory kind)");
    m.def("comm_open", &comm_open, "(handle, device) -> mapped address of a peer's buffer");
    m.def("comm_close", &comm_close, "unmap a peer's buffer");
    m.def("comm_free", &comm_free, "free the own buffer");
    m.def("comm_status", &comm_status, "(own buffer) -> [epoch, busy, status, lanes timed out]  (synchronous)");
    m.def("comm_clear_status", &comm_clear_status, "(own buffer): zero the sticky status word and the timed-out lane count (synchronous)");
    m.def("allreduce_oneshot", &allreduce_oneshot,
          "one-shot all-reduce of f32 partials over peer-mapped slots: (partial, peers, rank, capacity, dtype, bias|None, residual|None, timeout_us)");
    m.def("quantize_fp4", &quantize_fp4, "blockwise FP4 quantiser: (W, blocksize) -> (packed, absmax)");
    m.def("dequantize_nf4", &dequantize_nf4, "NF4 -> T dequant: (A, absmax, blocksize, M, N, o_type)");
    m.def("gemv_nf4", &gemv_nf4, "fused batch-1 NF4 GEMV: (A, B, absmax, blocksize, dtype, Bshape)");
    m.def("gemv_nf4_bias", &gemv_nf4_bias, "gemv_nf4 with the bias add fused into the epilogue: (A, B, absmax, blocksize, dtype, Bshape, bias)");
    m.def("qlinear_nf4", &qlinear_nf4, "NF4 dequant + linear: (A_in, A, absmax, M, N, blocksize)");
    m.def("qlinear_nf4_bias", &qlinear_nf4_bias, "NF4 dequant + linear + bias: (A_in, A, absmax, M, N, blocksize, bias)");
    m.def("gemm_small_nf4", &gemm_small_nf4, "fused NF4 product for 1..16 activation rows: (A, B, absmax, blocksize, Bshape, bias|None)");
    m.def("gemm_wide_nf4", &gemm_wide_nf4, "fused NF4 product for 1..128 activation rows: (A, B, absmax, blocksize, Bshape, bias|None)");
    m.def("gemv_nf4_fused", &gemv_nf4_fused,
          "NF4 GEMV with a fused epilogue: (A, B, absmax, blocksize, Bshape, bias|None, residual|None, epilogue) ; epilogue 0 = bias/residual, "
          "1 = silu(gate) * up over interleaved rows");
    m.def("gemm_nf4_fused", &gemm_nf4_fused,
          "fused NF4 product for 1..128 rows with an epilogue: (A, B, absmax, blocksize, Bshape, bias|None, residual|None, epilogue)");
    m.def("lora_down", &lora_down, "LoRA down projection: (x, A [R, K], scale float32 [R]) -> t = scale * (x @ A^T), float32 [rows, R]");
    m.def("gemv_nf4_lora", &gemv_nf4_lora,
          "gemv_nf4_fused plus the adapter term lora_B @ t in f32 before the rounding: (A, B, absmax, blocksize, Bshape, bias|None, "
          "residual|None, epilogue, lora_B [m, R], t float32 [1, R])");
    m.def("gemm_nf4_lora", &gemm_nf4_lora,
          "gemm_nf4_fused for 1..64 rows plus the adapter term: (A, B, absmax, blocksize, Bshape, bias|None, residual|None, epilogue, "
          "lora_B [m, R], t float32 [rows, R])");
    m.def("lora_down_multi", &lora_down_multi,
          "LoRA down projection with the adapter chosen per row on the device: (x, A_stack [n, R, K], scale_stack float32 [n, R], ids int32 "
          "[>= rows]) -> t float32 [rows, R]; +0 where ids[b] is outside 0..n-1");
    m.def("gemv_nf4_lora_multi", &gemv_nf4_lora_multi,
          "gemv_nf4_lora over a stack of adapters: (A, B, absmax, blocksize, [m, k] of the weight, bias|None, residual|None, epilogue, "
          "B_stack [n, m, R], ids int32 [>= 1], t float32 [1, R]); an id outside 0..n-1 gives gemv_nf4_fused");
    m.def("gemm_nf4_lora_multi", &gemm_nf4_lora_multi,
          "gemm_nf4_lora over a stack of adapters, one id per activation row: (A, B, absmax, blocksize, [m, k] of the weight, bias|None, "
          "residual|None, epilogue, B_stack [n, m, R], ids int32 [>= rows], t float32 [rows, R]); rows whose id is outside 0..n-1 are "
          "gemm_nf4_fused's");
    m.def("absmax_unnest", &absmax_unnest,
          "expand double-quantised absmax: (absmax_u8, nested_absmax, nested_code [256], offset, nested_blocksize) -> float32 [nb]");
    m.def("absmax_nest", &absmax_nest,
          "double-quantise absmax: (absmax float32 [nb], offset, nested_code [256], nested_blocksize) -> (absmax_u8, nested_absmax)");
    m.def("gemv_nf4_nested", &gemv_nf4_nested,
          "gemv_nf4_fused reading double-quantised absmax: (A, B, absmax_u8, nested_absmax, nested_code, offset, nested_blocksize, blocksize, "
          "Bshape, bias|None, residual|None, epilogue)");
    m.def("gemm_nf4_nested", &gemm_nf4_nested,
          "gemm_nf4_fused reading double-quantised absmax: (A, B, absmax_u8, nested_absmax, nested_code, offset, nested_blocksize, blocksize, "
          "[m, k] of the weight, bias|None, residual|None, epilogue)");
    m.def("gemv_nf4_lora_nested", &gemv_nf4_lora_nested,
          "gemv_nf4_lora reading double-quantised absmax: (A, B, absmax_u8, nested_absmax, nested_code, offset, nested_blocksize, blocksize, "
          "[m, k] of the weight, bias|None, residual|None, epilogue, lora_B [m, R], t float32 [1, R])");
    m.def("gemm_nf4_lora_nested", &gemm_nf4_lora_nested,
          "gemm_nf4_lora reading double-quantised absmax: (A, B, absmax_u8, nested_absmax, nested_code, offset, nested_blocksize, blocksize, "
          "[m, k] of the weight, bias|None, residual|None, epilogue, lora_B [m, R], t float32 [rows, R])");
    m.def("qlinear_nf4_nested", &qlinear_nf4_nested,
          "absmax_unnest + NF4 dequant + linear: (A_in, A, absmax_u8, nested_absmax, nested_code, offset, nested_blocksize, M, N, blocksize, bias|None)");
    m.def("quantize_nf4", &quantize_nf4, "blockwise NF4 quantiser: (W, blocksize) -> (packed, absmax)");
    m.def("code_table", &code_table, "16-entry code table as a CPU float tensor");
    m.def("set_kernel_variant", &set_kernel_variant, "benchmark hook: select a kernel geometry");
    m.def("set_qlinear_gemm", &set_qlinear_gemm,
          "which dense GEMM the qlinear* ops call after the dequant: 'hipblaslt' (direct, cached plans; default) or 'aten' (at::linear); "
          "returns the previous setting");
    m.def("qlinear_gemm_stats", &qlinear_gemm_stats,
          "calls of the qlinear* ops served by each GEMM route since the process started: {'direct': n, 'aten': n}");
    m.attr("EPILOGUE_NONE") = (int)FP4_EPILOGUE_NONE;
    m.attr("EPILOGUE_SILU_MUL_PAIRS") = (int)FP4_EPILOGUE_SILU_MUL_PAIRS;
    m.attr("abi_version") = fp4_hip_abi_version();
}
