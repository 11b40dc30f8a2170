// Stand-alone memory and undefined-behaviour check of the CPU build of the reference kernels.  TEST INFRASTRUCTURE ONLY.
// Built together with ref_entry.cpp under -fsanitize=address,undefined -fno-sanitize-recover=undefined by oracle/ref_cpu.py and run
// as a program of its own (tests/test_reference_vectors_host.py): nothing sanitized is ever loaded into python.
//
// It runs every entry point over the shapes of tests/golden/make_reference_vectors.py with operands of exactly the documented sizes
// (heap vectors, so that a read or write one element past an end is an AddressSanitizer report) and with the edge values of that
// generator in the scales and activations.  It checks no numbers: those are the business of the committed vectors.
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <limits>
#include <vector>

extern "C" {
int ref_flavour(void);
int ref_code_param(int which_file, float *out16);
int ref_dequant(int kernel, int dtype, const unsigned char *packed, const float *absmax, void *out, int blocksize, int n);
int ref_gemv(int dtype, const void *x, const unsigned char *packed, const float *absmax, void *out, int M, int K, int blocksize);
}

static uint32_t rng_state = 12345;
static uint32_t rnd() {  // xorshift32
    rng_state ^= rng_state << 13;
    rng_state ^= rng_state >> 17;
    rng_state ^= rng_state << 5;
    return rng_state;
}

static const float kEdges[] = {0.0f, 1e-41f, std::numeric_limits<float>::max(), std::numeric_limits<float>::infinity(),
                               std::numeric_limits<float>::quiet_NaN(), -0.75f};
static const int kDtypeSize[] = {2, 4, 2};  // f16, f32, bf16

static std::vector<float> scales(size_t n, bool edges) {
    std::vector<float> a(n);
    for (size_t i = 0; i < n; i++) a[i] = std::ldexp(1.0f + (rnd() % 1024) / 1024.0f, (int)(rnd() % 40) - 25);
    if (edges)
        for (size_t i = 0; i < n; i++)
            if (i % 3 == 1) a[i] = kEdges[(i / 3) % 6];
    return a;
}

static int fail(const char *what, int a, int b, int c, int d) {
    std::fprintf(stderr, "selfcheck: %s failed at (%d, %d, %d, %d)\n", what, a, b, c, d);
    return 1;
}

int main() {
    float table[16];
    for (int f = 0; f < 2; f++)
        if (ref_code_param(f, table) != 0 || table[3] != 1.0f || table[11] != -1.0f) return fail("ref_code_param", f, 0, 0, 0);
    if (ref_code_param(2, table) == 0) return fail("ref_code_param range", 2, 0, 0, 0);

    // the grid's lengths; then those of the generator's other cases: 8 * bs + 3 ("edges"), 1040 and 8192 ("bytes" at blocksize 40 and
    // 4096; 1024 and 16, "codes at scale 1", are in the grid) and the long cases' 32768 + 16384 + 77 - each at every blocksize, since
    // n and blocksize together decide how far the idle threads of the last tile reach
    const int lengths[] = {1, 2, 15, 16, 17, 1023, 1024, 1025, 2050, 3333, 259, 515, 1040, 8192, 32768 + 16384 + 77};
    const int blocksizes[] = {32, 40, 64, 128, 256, 4096};
    long runs = 0;
    for (int n : lengths)
        for (int bs : blocksizes) {
            std::vector<unsigned char> packed((n + 1) / 2);
            for (auto &b : packed) b = (unsigned char)rnd();
            std::vector<float> am = scales((size_t)(n + bs - 1) / bs, true);
            for (int kernel = 0; kernel < 2; kernel++)
                for (int dt = 0; dt < 3; dt++) {
                    std::vector<unsigned char> out((size_t)n * kDtypeSize[dt], 0xA5);
                    if (ref_dequant(kernel, dt, packed.data(), am.data(), out.data(), bs, n) != 0) return fail("ref_dequant", n, bs, kernel, dt);
                    runs++;
                }
        }

    const int shapes[][3] = {{5, 32, 64},   {6, 96, 32},    {7, 1024, 64}, {6, 1056, 64}, {3, 2080, 128},
                             {2, 4096, 64}, {9, 3104, 4096}, {4, 32, 32},   {1, 64, 64},   {13, 992, 32}};
    for (auto &s : shapes) {
        const int M = s[0], K = s[1], bs = s[2];
        std::vector<unsigned char> packed((size_t)M * K / 2);
        for (auto &b : packed) b = (unsigned char)rnd();
        for (int edges = 0; edges < 2; edges++) {
            std::vector<float> am = scales(((size_t)M * K + bs - 1) / bs, edges != 0);
            for (int dt = 0; dt < 3; dt++) {
                // activations: arbitrary bit patterns of the type are all legal inputs (NaN, Inf and subnormals among them)
                std::vector<unsigned char> x((size_t)K * kDtypeSize[dt]);
                for (auto &b : x) b = (unsigned char)rnd();
                if (!edges) std::memset(x.data(), 0, x.size() / 2);  // and once with a run of zeros in front
                std::vector<unsigned char> out((size_t)M * kDtypeSize[dt], 0xA5);
                if (ref_gemv(dt, x.data(), packed.data(), am.data(), out.data(), M, K, bs) != 0) return fail("ref_gemv", M, K, bs, dt);
                runs++;
            }
        }
    }
    if (ref_gemv(1, table, nullptr, nullptr, table, 4, 48, 32) == 0) return fail("ref_gemv must refuse K % 32 != 0", 4, 48, 32, 1);
    std::printf("selfcheck ok: flavour %d, %ld kernel launches\n", ref_flavour(), runs);
    return 0;
}
