// CPU stand-in for the parts of CUDA, CUB and cooperative_groups that the reference's two kernel files use.
// TEST INFRASTRUCTURE ONLY.  All of this is the project's own text; the reference's kernel text is compiled against it unedited
// (oracle/ref_cpu.py cuts it out of a reference checkout into oracle/_ref/, which is never committed).
//
// Execution model: one OS thread per CUDA thread, one thread block at a time.  `__shared__` becomes `static`, which is shared by
// the threads of the running block because blocks never overlap; `__syncthreads()` is a std::barrier over the block.
#pragma once
#include <barrier>
#include <cfloat>
#include <climits>
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <functional>
#include <iostream>
#include <limits.h>
#include <map>
#include <memory>
#include <mutex>
#include <stdio.h>
#include <thread>
#include <vector>

// ---- qualifiers ----------------------------------------------------------------------------------------------------------------------
#define __global__
#define __device__
#define __host__
#define __forceinline__ inline
#define __shared__ static  // one block runs at a time (ref_launch below), so a function-local static IS the block's shared memory
#define __grid_constant__  // a by-value kernel parameter: nothing to emulate

// ---- built-in variables (CUDA C++ Programming Guide, "Built-in Variables"): unsigned, as the index arithmetic of
// dequant_fp4_optimized.cu:108-110 mixes them with int and the usual arithmetic conversions decide the result ----------------------------
struct ref_uint3 {
    unsigned int x, y, z;
};
inline thread_local ref_uint3 threadIdx{0, 0, 0}, blockIdx{0, 0, 0}, blockDim{1, 1, 1}, gridDim{1, 1, 1};
inline thread_local std::barrier<> *ref_block_barrier = nullptr;

inline void __syncthreads() { ref_block_barrier->arrive_and_wait(); }

// kernel<<<grid, block>>>(...): `block` OS threads run the body for block 0, then together for block 1, ...
// The threads of a block size are started once and kept for later launches (starting 64 or 128 threads per launch dominates the
// run time otherwise, under a sanitizer above all); the caller's thread hands them a launch and waits for it.
class ref_thread_pool {
    const unsigned block;
    std::barrier<> in_block, hand_over;  // among the block's threads; between them and the launching thread
    std::function<void()> body;
    unsigned grid = 0;
    bool stop = false;
    std::vector<std::thread> threads;

    void worker(unsigned t) {
        threadIdx = {t, 0, 0};
        blockDim = {block, 1, 1};
        ref_block_barrier = &in_block;
        for (;;) {
            hand_over.arrive_and_wait();  // a launch (or the end) has been posted
            if (stop) return;
            gridDim = {grid, 1, 1};
            for (unsigned b = 0; b < grid; b++) {
                blockIdx = {b, 0, 0};
                body();
                in_block.arrive_and_wait();  // the next block reuses the statics that stand for shared memory
            }
            hand_over.arrive_and_wait();  // launch finished
        }
    }

public:
    explicit ref_thread_pool(unsigned block_) : block(block_), in_block(block_), hand_over(block_ + 1) {
        for (unsigned t = 0; t < block; t++) threads.emplace_back([this, t] { worker(t); });
    }
    ~ref_thread_pool() {
        stop = true;
        hand_over.arrive_and_wait();
        for (auto &th : threads) th.join();
    }
    void run(unsigned grid_, std::function<void()> body_) {
        grid = grid_;
        body = std::move(body_);
        hand_over.arrive_and_wait();
        hand_over.arrive_and_wait();
    }
};

inline void ref_launch(unsigned grid, unsigned block, std::function<void()> body) {
    static std::mutex one_launch_at_a_time;
    static std::map<unsigned, std::unique_ptr<ref_thread_pool>> pools;
    std::lock_guard<std::mutex> lock(one_launch_at_a_time);
    auto &pool = pools[block];
    if (!pool) pool = std::make_unique<ref_thread_pool>(block);
    pool->run(grid, std::move(body));
}

template <class T> inline T __ldg(const T *p) { return *p; }  // a read-only cached load is a load

// the 16-byte vector type: the reference loads it through `unsigned char[16]` locals and at addresses that are only byte aligned
// as far as C++ knows (gemv_fp4_optimized.cu:107-108,133), so it is packed (alignment 1) and may alias anything
struct __attribute__((packed, may_alias)) int4 {
    int x, y, z, w;
};

typedef int cudaError_t;
constexpr cudaError_t cudaSuccess = 0;
inline const char *cudaGetErrorString(cudaError_t) { return "no CUDA here"; }
inline cudaError_t cudaGetLastError() { return cudaSuccess; }

// ---- 16-bit floating types -----------------------------------------------------------------------------------------------------------
// IEEE round-to-nearest-even of a double to a format with MANT stored mantissa bits and exponent bias BIAS, subnormals kept
// (what __float2half_rn / __float2bfloat16_rn and the 16-bit arithmetic instructions do for finite results).  NaN comes out as one
// canonical quiet NaN: NVIDIA's payloads are not in the reference's text, and every comparison treats NaN by class.
template <int MANT, int BIAS> inline uint16_t ref_round_bits(double v) {
    const uint16_t exp_all = (uint16_t)(((1u << (15 - MANT)) - 1) << MANT);
    if (std::isnan(v)) return (uint16_t)(exp_all | (1u << (MANT - 1)));
    const uint16_t sign = std::signbit(v) ? 0x8000 : 0;
    double a = std::fabs(v);
    if (std::isinf(a)) return sign | exp_all;
    if (a == 0.0) return sign;
    int e;
    std::frexp(a, &e);  // a = m * 2^e, 0.5 <= m < 1
    int E = e - 1;
    const int emin = 1 - BIAS;
    if (E < emin) E = emin;
    double q = std::ldexp(a, MANT - E);  // exact: a power-of-two scaling well inside double's range
    double r = std::nearbyint(q);        // default rounding mode: to nearest, ties to even
    uint32_t ri = (uint32_t)r;
    if (ri >= (2u << MANT)) {
        ri >>= 1;
        E++;
    }
    if (E > BIAS) return sign | exp_all;  // rounded past the largest finite value
    if (ri < (1u << MANT)) return sign | (uint16_t)ri;  // subnormal (E == emin)
    return sign | (uint16_t)(((uint32_t)(E + BIAS) << MANT) | (ri - (1u << MANT)));
}

template <int MANT, int BIAS> inline float ref_bits_value(uint16_t b) {
    const int ebits = 15 - MANT;
    const uint32_t e = (b >> MANT) & ((1u << ebits) - 1), m = b & ((1u << MANT) - 1);
    float v;
    if (e == (1u << ebits) - 1) v = m ? NAN : INFINITY;
    else if (e == 0) v = std::ldexp((float)m, 1 - BIAS - MANT);
    else v = std::ldexp((float)(m | (1u << MANT)), (int)e - BIAS - MANT);
    return (b & 0x8000) ? -v : v;
}

// Helper for the contracted flavour: p + c rounded ONCE to the 16-bit format.  p is an exact product held in a double;
// the double sum is corrected to round-to-odd (Boldo & Melquiond, "Emulation of FMA and correctly rounded sums", 2008) so that
// the second rounding to 8 or 11 bits cannot double-round.
inline double ref_add_round_to_odd(double p, double c) {
    double s = p + c;
    if (!std::isfinite(s)) return s;
    double bb = s - p, err = (p - (s - bb)) + (c - bb);  // TwoSum: s + err == p + c exactly
    if (err == 0.0) return s;
    uint64_t u;
    std::memcpy(&u, &s, 8);
    if ((u & 1) == 0) {
        // s is even and inexact: step to the odd neighbour on the side of the exact sum
        const bool away = (err > 0) == (s > 0);
        u = away ? u + 1 : u - 1;
        std::memcpy(&s, &u, 8);
    }
    return s;
}

template <int MANT, int BIAS> struct ref_f16 {
    uint16_t bits;
    ref_f16() = default;
    ref_f16(float f) : bits(ref_round_bits<MANT, BIAS>((double)f)) {}  // __float2half_rn / __float2bfloat16_rn; also `T x = float`
    operator float() const { return ref_bits_value<MANT, BIAS>(bits); }  // __half2float: exact
    static ref_f16 from_double(double d) {
        ref_f16 r;
        r.bits = ref_round_bits<MANT, BIAS>(d);
        return r;
    }
};

#ifndef REF_CONTRACT_FMA
// cuda_fp16.hpp / cuda_bf16.hpp: operator* is __hmul, operator+= is __hadd; each rounds its result to the 16-bit format.  A
// product of two such values is exact in a double, so rounding the double product once is the instruction's rounding.
template <int M, int B> inline ref_f16<M, B> operator*(ref_f16<M, B> a, ref_f16<M, B> b) {
    return ref_f16<M, B>::from_double((double)(float)a * (double)(float)b);
}
template <int M, int B> inline ref_f16<M, B> &operator+=(ref_f16<M, B> &a, ref_f16<M, B> b) {
    // the double sum is exact unless the operands lie more than 40 binades apart, and then the result is the larger operand, which
    // is already on the 16-bit grid: one rounding either way
    a = ref_f16<M, B>::from_double((double)(float)a + (double)(float)b);
    return a;
}
#else
// The other thing a CUDA compiler may emit for `local_C += a * b` (gemv_fp4_optimized.cu:147): one __hfma, a single rounding.
// operator* yields an unrounded product; assigning it rounds (local_B = quant_map * absmax, :128-129), adding it to an
// accumulator fuses.
template <int M, int B> struct ref_prod {
    double exact;
    operator ref_f16<M, B>() const { return ref_f16<M, B>::from_double(exact); }
};
template <int M, int B> inline ref_prod<M, B> operator*(ref_f16<M, B> a, ref_f16<M, B> b) {
    return {(double)(float)a * (double)(float)b};
}
template <int M, int B> inline ref_f16<M, B> &operator+=(ref_f16<M, B> &a, ref_prod<M, B> p) {
    a = ref_f16<M, B>::from_double(ref_add_round_to_odd(p.exact, (double)(float)a));
    return a;
}
#endif

typedef ref_f16<10, 15> nv_half;       // IEEE binary16
typedef ref_f16<7, 127> nv_bfloat16;   // bfloat16
typedef nv_half __half, half;
typedef nv_bfloat16 __nv_bfloat16;
inline nv_half __float2half_rn(float f) { return nv_half(f); }
inline nv_bfloat16 __float2bfloat16_rn(float f) { return nv_bfloat16(f); }

// ---- cooperative_groups: only this_thread_block().thread_rank() is used (dequant_fp4_optimized.cu:138,150-151) ----------------------------
namespace cooperative_groups {
struct thread_block {
    unsigned thread_rank() const { return threadIdx.x; }
};
inline thread_block this_thread_block() { return {}; }
}  // namespace cooperative_groups

// ---- CUB ---------------------------------------------------------------------------------------------------------------------------------
namespace cub {
enum BlockLoadAlgorithm { BLOCK_LOAD_DIRECT, BLOCK_LOAD_WARP_TRANSPOSE };
enum BlockStoreAlgorithm { BLOCK_STORE_DIRECT, BLOCK_STORE_WARP_TRANSPOSE };

// cub::BlockLoad, guarded overload with an out-of-bounds default (cub/block/block_load.cuh).  BLOCK_LOAD_WARP_TRANSPOSE reads a
// warp-striped arrangement and transposes it, so what the caller sees is the BLOCKED arrangement: thread t holds items
// [t * ITEMS, (t + 1) * ITEMS).  The staging through shared memory has no arithmetic effect and is not emulated.
template <class T, int THREADS, int ITEMS, BlockLoadAlgorithm ALG> struct BlockLoad {
    struct TempStorage {};
    BlockLoad(TempStorage &) {}
    template <class It, class D> void Load(It src, T (&items)[ITEMS], int valid_items, D oob_default) {
        for (int j = 0; j < ITEMS; j++) {
            int idx = (int)threadIdx.x * ITEMS + j;
            items[j] = idx < valid_items ? src[idx] : (T)oob_default;
        }
    }
};

// cub::BlockStore, guarded overload (cub/block/block_store.cuh): blocked arrangement in, items past valid_items are not written.
template <class T, int THREADS, int ITEMS, BlockStoreAlgorithm ALG> struct BlockStore {
    struct TempStorage {};
    BlockStore(TempStorage &) {}
    template <class It> void Store(It dst, T (&items)[ITEMS], int valid_items) {
        for (int j = 0; j < ITEMS; j++) {
            int idx = (int)threadIdx.x * ITEMS + j;
            if (idx < valid_items) dst[idx] = items[j];
        }
    }
};

// cub::WarpReduce<float>::Sum over a full 32-lane warp (cub/warp/specializations/warp_reduce_shfl.cuh): for offsets 1, 2, 4, 8,
// 16 every lane fetches the value of lane + offset (shfl.down) and adds it if that lane exists; lane 0 ends with the total.  The
// exchange goes through the TempStorage the caller hands in; every thread of the block calls Sum together (gemv_fp4_optimized.cu:152,
// outside every branch), so the block barrier orders the exchange.
template <class T> struct WarpReduce {
    struct TempStorage {
        T lane_value[32];
    };
    TempStorage &s;
    WarpReduce(TempStorage &t) : s(t) {}
    T Sum(T v) {
        const unsigned lane = threadIdx.x % 32;
        for (unsigned offset = 1; offset < 32; offset *= 2) {
            s.lane_value[lane] = v;
            __syncthreads();
            const bool in_range = lane + offset < 32;
            const T other = in_range ? s.lane_value[lane + offset] : T(0);
            __syncthreads();
            if (in_range) v = v + other;
        }
        return v;
    }
};
}  // namespace cub
