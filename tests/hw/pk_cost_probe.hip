// Hardware probe (not a test): what does ONE VALU instruction of a given kind cost when it is issued between the
// v_mfma_f32_16x16x32_bf16 of the AR_X3 point kernel - at one AND at two waves per SIMD?  
//
// The packed fp32 forms (v_pk_fma_f32 / v_pk_mul_f32 / v_pk_add_f32) were priced by the project only between fp32 16x16x4 MFMAs
// (mfma_overlap_probe.hip: 7.6 cycles = two scalar ones) and v_dot2c_f32_bf16 only in a stream without any MFMA
// (valu_cost_probe.hip).  This probe prices them where the product kernel issues them.
//
// Stream of a wave: the chain mfma_unit3 issues - six v_mfma_f32_16x16x32_bf16 back to back on one accumulator, then six on the
// other slot's accumulator, repeated - with N = 0, 1, 2, 4 filler UNITS of one type after every MFMA (in its "gap").  A unit is
//   fma2    2 x v_fma_f32               pk_fma  1 x v_pk_fma_f32        (the same two results)
//   mul2    2 x v_mul_f32               pk_mul  1 x v_pk_mul_f32
//   add2    2 x v_add_f32               pk_add  1 x v_pk_add_f32
//   dot2    1 x v_dot2c_f32_bf16        shsub   v_lshlrev_b32 + v_sub_f32   (the unpack + subtract the dot product replaced)
//   exp     1 x v_exp_f32               cvt     1 x v_cvt_pk_bf16_f32       (known references)
// Fillers run on 8 independent registers (pairs) in turn, so no filler waits for the one before it.  Plain and packed fp32
// arithmetic is inline asm (nothing for the compiler to re-pack or fuse; VALU -> VALU needs no software wait states); the dot
// product, the exponential and the conversion are BUILTINS, because their results need wait states before the next reader that
// only the compiler's hazard recogniser inserts (nr_platform.h, nr_split3) - and the selector pair of the dot product comes out
// of an opaque s_mov so that it is not folded into the inline constant -1.0 (dot2_residual_probe.hip).  sched_barriers pin the
// order MFMA, fillers, MFMA, ...
//
// Modes: A one wave per SIMD (workgroups of 256 threads, one per CU) | B two waves per SIMD, both run the stream |
//        C two waves per SIMD, the partner runs a VALU-only stream (independent v_fma_f32) until the stream waves are done.
// Reported: SIMD cycles per MFMA gap of a stream wave (constant-rate wall clock of the stream waves, nominal shader clock),
// median of 3 launches, and the cost of one filler unit = (t(N) - t(0)) / N.
//
//   hipcc --offload-arch=gfx950 -O3 -ffp-contract=off tests/hw/pk_cost_probe.hip -o tests/hw/pk_cost_probe && tests/hw/pk_cost_probe
#include <hip/hip_runtime.h>
#include <algorithm>
#include <cstdio>
#include <cstdlib>
#include <vector>

typedef float v4f __attribute__((ext_vector_type(4)));
typedef float v2f __attribute__((ext_vector_type(2)));
typedef unsigned int v4u __attribute__((ext_vector_type(4)));
typedef __bf16 v8bf __attribute__((ext_vector_type(8)));
typedef __bf16 v2bf __attribute__((ext_vector_type(2)));

#define CHECK(x) do { hipError_t e_ = (x); if (e_ != hipSuccess) { printf("HIP error %s at %s:%d\n", hipGetErrorString(e_), __FILE__, __LINE__); exit(1); } } while (0)

enum Fill { FMA2, PK_FMA, MUL2, PK_MUL, ADD2, PK_ADD, DOT2, SHSUB, EXP, CVT, NFILL };
static const char* kFill[NFILL] = {"fma2   2 x v_fma_f32", "pk_fma 1 x v_pk_fma_f32", "mul2   2 x v_mul_f32", "pk_mul 1 x v_pk_mul_f32", "add2   2 x v_add_f32",
                                   "pk_add 1 x v_pk_add_f32", "dot2   1 x v_dot2c_f32_bf16", "shsub  v_lshlrev + v_sub_f32", "exp    1 x v_exp_f32", "cvt    1 x v_cvt_pk_bf16_f32"};

struct Regs {
    float f[8];
    v2f p[8];
    float one, zero;          // multiplier / addend that leave the values where they are
    v2f one2, zero2;
    unsigned h;               // a bf16 pair
    v2bf klo;                 // selector pair (-1, 0)
};

template <int F>
__device__ __forceinline__ void filler(Regs& r, int j) {
    const int a = j & 3, b = 4 + (j & 3), k = j & 7;
    if constexpr (F == FMA2) asm volatile("v_fma_f32 %0, %0, %2, %3\n\tv_fma_f32 %1, %1, %2, %3" : "+v"(r.f[a]), "+v"(r.f[b]) : "v"(r.one), "v"(r.zero));
    if constexpr (F == PK_FMA) asm volatile("v_pk_fma_f32 %0, %0, %1, %2" : "+v"(r.p[k]) : "v"(r.one2), "v"(r.zero2));
    if constexpr (F == MUL2) asm volatile("v_mul_f32 %0, %0, %2\n\tv_mul_f32 %1, %1, %2" : "+v"(r.f[a]), "+v"(r.f[b]) : "v"(r.one));
    if constexpr (F == PK_MUL) asm volatile("v_pk_mul_f32 %0, %0, %1" : "+v"(r.p[k]) : "v"(r.one2));
    if constexpr (F == ADD2) asm volatile("v_add_f32 %0, %0, %2\n\tv_add_f32 %1, %1, %2" : "+v"(r.f[a]), "+v"(r.f[b]) : "v"(r.zero));
    if constexpr (F == PK_ADD) asm volatile("v_pk_add_f32 %0, %0, %1" : "+v"(r.p[k]) : "v"(r.zero2));
    if constexpr (F == DOT2) r.f[k] = __builtin_amdgcn_fdot2_f32_bf16(__builtin_bit_cast(v2bf, r.h), r.klo, r.f[k], false);
    if constexpr (F == SHSUB) {
        float t;
        asm volatile("v_lshlrev_b32 %1, 16, %2\n\tv_sub_f32 %0, %0, %1" : "+v"(r.f[k]), "=&v"(t) : "v"(r.h));
    }
    if constexpr (F == EXP) r.f[k] = __builtin_amdgcn_exp2f(r.f[k]);
    if constexpr (F == CVT) {
        v2bf v; v[0] = (__bf16)r.f[k]; v[1] = (__bf16)r.f[k ^ 1];
        r.f[k] = __builtin_bit_cast(float, v);
    }
}

// the VALU-only partner of mode C: independent v_fma_f32 until the four stream waves of the workgroup are done
__device__ __forceinline__ void valu_partner(const float* in, float* out, volatile int* done, int lane) {
    float g[8];
    for (int k = 0; k < 8; ++k) g[k] = in[lane + k];
    const float one = in[64], zero = in[65];
    while (true) {
#pragma unroll
        for (int i = 0; i < 16; ++i)
            asm volatile("v_fma_f32 %0, %0, %8, %9\n\tv_fma_f32 %1, %1, %8, %9\n\tv_fma_f32 %2, %2, %8, %9\n\tv_fma_f32 %3, %3, %8, %9\n\t"
                         "v_fma_f32 %4, %4, %8, %9\n\tv_fma_f32 %5, %5, %8, %9\n\tv_fma_f32 %6, %6, %8, %9\n\tv_fma_f32 %7, %7, %8, %9"
                         : "+v"(g[0]), "+v"(g[1]), "+v"(g[2]), "+v"(g[3]), "+v"(g[4]), "+v"(g[5]), "+v"(g[6]), "+v"(g[7]) : "v"(one), "v"(zero));
        if (*done >= 4) break;
    }
    float s = 0.f;
    for (int k = 0; k < 8; ++k) s += g[k];
    if (s == 123.456f) out[lane] = s;
}

// mode 0 / 1: every wave runs the stream (256 / 512 threads); mode 2: waves 4..7 are VALU partners
template <int F, int N>
__global__ void __launch_bounds__(512) stream(const float* in, unsigned long long* ticks, float* out, int iters, int mode) {
    __shared__ int done;
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    if (threadIdx.x == 0) done = 0;
    __syncthreads();
    if (mode == 2 && wave >= 4) { valu_partner(in, out, &done, lane); return; }
    Regs r;
    for (int k = 0; k < 8; ++k) { r.f[k] = in[lane + k]; r.p[k] = (v2f){in[lane + k], in[lane + k + 8]}; }
    r.one = in[64]; r.zero = in[65];
    r.one2 = (v2f){in[64], in[64]}; r.zero2 = (v2f){in[65], in[65]};
    r.h = __builtin_bit_cast(unsigned, in[66 + (lane & 1)]);
    unsigned klo_;
    asm("s_mov_b32 %0, 0xbf80" : "=s"(klo_));
    r.klo = __builtin_bit_cast(v2bf, klo_);
    v4u a = {lane * 3u + 1u, lane * 5u + 2u, lane * 7u + 3u, lane * 11u + 4u}, b = a;
    a[0] &= 0x3f803f80u; a[1] &= 0x3f803f80u; a[2] &= 0x3f803f80u; a[3] &= 0x3f803f80u;      // small finite bf16 values
    b = a; b[0] ^= 0x00800000u;
    v4f acc[2] = {{0.f, 0.f, 0.f, 0.f}, {0.f, 0.f, 0.f, 0.f}};
    const unsigned long long t0 = wall_clock64();
    for (int it = 0; it < iters; ++it) {
#pragma unroll
        for (int s = 0; s < 2; ++s)
#pragma unroll
            for (int q = 0; q < 6; ++q) {
                acc[s] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(__builtin_bit_cast(v8bf, a), __builtin_bit_cast(v8bf, b), acc[s], 0, 0, 0);
                __builtin_amdgcn_sched_barrier(0);
#pragma unroll
                for (int k = 0; k < N; ++k) filler<F>(r, (s * 6 + q) * N + k);
                __builtin_amdgcn_sched_barrier(0);
            }
    }
    const unsigned long long t1 = wall_clock64();
    if (lane == 0) { ticks[blockIdx.x * 8 + wave] = t1 - t0; atomicAdd(&done, 1); }
    float sum = 0.f;
    for (int k = 0; k < 8; ++k) sum += r.f[k] + r.p[k].x + r.p[k].y;
    for (int s = 0; s < 2; ++s) sum += acc[s][0] + acc[s][1] + acc[s][2] + acc[s][3];
    if (sum == 123.456f) out[threadIdx.x] = sum;
}

struct Ctx { float* in; unsigned long long* ticks; float* out; int cus; double ghz, wall_hz; };
static const int kIters = 20000;

template <int F, int N>
static double gap_cycles(const Ctx& c, int mode) {
    const int threads = mode == 0 ? 256 : 512, nstream = mode == 1 ? 8 : 4;
    std::vector<unsigned long long> t((size_t)c.cus * 8);
    double med[3];
    for (int rep = 0; rep < 3; ++rep) {
        CHECK(hipMemset(c.ticks, 0, t.size() * 8));
        hipLaunchKernelGGL((stream<F, N>), c.cus, threads, 0, 0, c.in, c.ticks, c.out, kIters, mode);
        CHECK(hipDeviceSynchronize());
        CHECK(hipMemcpy(t.data(), c.ticks, t.size() * 8, hipMemcpyDeviceToHost));
        double sum = 0;
        for (int blk = 0; blk < c.cus; ++blk) for (int w = 0; w < nstream; ++w) sum += (double)t[blk * 8 + w];
        med[rep] = sum / ((double)c.cus * nstream) / c.wall_hz * c.ghz * 1e9 / ((double)kIters * 12);
    }
    std::sort(med, med + 3);
    return med[1];
}

template <int F>
static void row(const Ctx& c, int mode) {
    const double t0 = gap_cycles<F, 0>(c, mode), t1 = gap_cycles<F, 1>(c, mode), t2 = gap_cycles<F, 2>(c, mode), t4 = gap_cycles<F, 4>(c, mode);
    printf("  %-30s N=0 %6.2f  N=1 %6.2f  N=2 %6.2f  N=4 %6.2f   per unit: %6.2f %6.2f %6.2f\n", kFill[F], t0, t1, t2, t4, t1 - t0, (t2 - t0) / 2, (t4 - t0) / 4);
}

int main() {
    Ctx c;
    hipDeviceProp_t prop;
    CHECK(hipGetDeviceProperties(&prop, 0));
    c.cus = prop.multiProcessorCount;
    c.ghz = prop.clockRate * 1e-6;
    int wall_khz = 0;
    CHECK(hipDeviceGetAttribute(&wall_khz, hipDeviceAttributeWallClockRate, 0));
    c.wall_hz = wall_khz * 1e3;
    std::vector<float> h(4096, 0.5f);
    h[64] = 1.0f; h[65] = 0.0f;
    const unsigned pair = 0x3f003e80u;             // bf16 (0.25, 0.5)
    h[66] = h[67] = __builtin_bit_cast(float, pair);
    CHECK(hipMalloc(&c.in, h.size() * 4));
    CHECK(hipMemcpy(c.in, h.data(), h.size() * 4, hipMemcpyHostToDevice));
    CHECK(hipMalloc(&c.ticks, (size_t)c.cus * 8 * 8));
    CHECK(hipMalloc(&c.out, 512 * 4));
    printf("%d CUs, nominal %.2f GHz, wall clock %.0f MHz; SIMD cycles per MFMA gap of a stream wave (6 + 6 v_mfma_f32_16x16x32_bf16 on two accumulators, N filler units per gap)\n",
           c.cus, c.ghz, c.wall_hz * 1e-6);
    static const char* kMode[3] = {"A: one wave per SIMD", "B: two waves per SIMD, both run the stream", "C: two waves per SIMD, the partner runs independent v_fma_f32 only"};
    for (int mode = 0; mode < 3; ++mode) {
        printf("%s\n", kMode[mode]);
        row<FMA2>(c, mode); row<PK_FMA>(c, mode); row<MUL2>(c, mode); row<PK_MUL>(c, mode); row<ADD2>(c, mode); row<PK_ADD>(c, mode);
        row<DOT2>(c, mode); row<SHSUB>(c, mode); row<EXP>(c, mode); row<CVT>(c, mode);
    }
    return 0;
}
