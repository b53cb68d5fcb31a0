// bsk.hip — on-device conversion of the standard u64 bootstrapping key into the exact-limb
// Fourier key consumed by pbs.hip.
//
// Reference: cuda_convert_lwe_programmable_bootstrap_key_64 as called by the runtime
// (compiler include/concretelang/Runtime/context.h:86-115); CPU counterpart
// concrete-cpu c_api/bootstrap.rs:241-318 (f64 Fourier conversion).  Here every key
// polynomial g (u64) is split into LIMBS balanced signed limbs, each limb is folded,
// twisted and transformed with a double-double (~106-bit) radix-2 FFT, so the stored f64
// spectrum is correctly rounded to within 1 ulp: the certified error bound of DESIGN.md §3
// charges only u * |G| for the key side.
//
// Input layout : [n][l][k+1 (row)][k+1 (col)][N] u64 (concrete-cpu bootstrap.rs:417-429)
// Output layout: [n][col][limb][row*l + q][k2][lane] complex f64, q = l-1-level_index,
//                frequency of (lane, k2) = fft512_freq(lane, k2), scaled by 2/N.
#include <cmath>
#include <mutex>
#include <vector>

#include "common.hpp"
#include "companion.hpp"
#include "fft512.hpp"
#include "keycheck.hpp"
#include "pbs.hpp"

// No FMA contraction in this file.  The double-double routines below are error-free transformations:
// they need p = rn(x y) and s = rn(p + e) as written.  Device code is compiled with -ffp-contract=fast,
// and the AMDGPU backend fuses a product into its uses even when it has several (quick_two_sum(p, e)
// became fma(x, y, e) and e - (fma(-x, y, s)), counting the product's rounding error twice): the stored
// spectra were then off by ~2^-56 of the block's largest value instead of correctly rounded
// (tests/test_gpu_key_accuracy.py).  The one fused operation that is meant is
// written as __builtin_fma.
#pragma clang fp contract(off)

namespace chip {

struct dd {
  double hi, lo;
};
__device__ __forceinline__ dd quick_two_sum(double a, double b) {
  double s = a + b;
  return {s, b - (s - a)};
}
__device__ __forceinline__ dd two_sum(double a, double b) {
  double s = a + b;
  double bb = s - a;
  return {s, (a - (s - bb)) + (b - bb)};
}
__device__ __forceinline__ dd dd_add(dd x, dd y) {
  dd s = two_sum(x.hi, y.hi);
  dd t = two_sum(x.lo, y.lo);
  s.lo += t.hi;
  s = quick_two_sum(s.hi, s.lo);
  s.lo += t.lo;
  return quick_two_sum(s.hi, s.lo);
}
__device__ __forceinline__ dd dd_neg(dd x) { return {-x.hi, -x.lo}; }
__device__ __forceinline__ dd dd_mul(dd x, dd y) {
  double p = x.hi * y.hi;
  double e = __builtin_fma(x.hi, y.hi, -p);
  e += x.hi * y.lo + x.lo * y.hi;
  return quick_two_sum(p, e);
}
__device__ __forceinline__ dd dd_from(double a) { return {a, 0.0}; }

struct ddc {
  dd re, im;
};
__device__ __forceinline__ ddc ddc_mul(ddc a, ddc w) {
  return {dd_add(dd_mul(a.re, w.re), dd_neg(dd_mul(a.im, w.im))), dd_add(dd_mul(a.re, w.im), dd_mul(a.im, w.re))};
}

// balanced signed limb `limb` of a 64-bit word (limb widths 64/LIMBS, the first 64 % LIMBS one
// bit wider: 22/21/21 for 3 limbs, 16 x 4 for 4): x = sum_t limb_t 2^{s_t} (mod 2^64)
template <int LIMBS>
__device__ __forceinline__ double limb_value(uint64_t rem, uint32_t limb) {
  int64_t lv = 0;
  for (int t = 0; t <= (int)limb; ++t) {
    int w = 64 / LIMBS + (t < 64 % LIMBS ? 1 : 0);
    uint64_t mask = (1ull << w) - 1ull;
    uint64_t vv = rem & mask;
    int64_t sgn = (vv >= (1ull << (w - 1))) ? (int64_t)vv - (int64_t)(1ull << w) : (int64_t)vv;
    lv = sgn;
    rem = (rem - (uint64_t)sgn) >> w;
  }
  return (double)lv;
}

constexpr int ilog2(int x) { return x <= 1 ? 0 : 1 + ilog2(x / 2); }

// The next digit of a mixed-radix block index, least significant first: t % radix, and t /= radix.
__device__ __forceinline__ uint32_t next_digit(uint64_t& t, uint32_t radix) {
  const uint32_t d = (uint32_t)(t % radix);
  t /= radix;
  return d;
}

// The M points the transform starts from: limb `limb` of the polynomial whose coefficient j is
// g[step * j], folded and twisted, z_j = (a_j + i a_{j+M}) * zeta^j, stored at the bit-reversed position
// for the DIT passes.
template <int M, int LIMBS>
__device__ __forceinline__ void load_twisted(ddc* buf, const uint64_t* __restrict__ g, int step, uint32_t limb,
                                             const ddc* __restrict__ zeta_t) {
  for (int j = threadIdx.x; j < M; j += blockDim.x) {
    ddc z{dd_from(limb_value<LIMBS>(g[step * j], limb)), dd_from(limb_value<LIMBS>(g[step * (j + M)], limb))};
    z = ddc_mul(z, zeta_t[j]);
    const int r = (int)(__builtin_bitreverse32((uint32_t)j) >> (32 - ilog2(M)));
    buf[r] = z;
  }
  __syncthreads();
}

// In-LDS radix-2 DIT over buf (bit-reversed input, natural output, forward sign)
template <int M>
__device__ __forceinline__ void dd_fft(ddc* buf, const ddc* __restrict__ tw_t) {
  for (int h = 1; h < M; h <<= 1) {
    for (int b = threadIdx.x; b < M / 2; b += blockDim.x) {
      const int grp = b / h, pos = b % h;
      const int i0 = grp * 2 * h + pos, i1 = i0 + h;
      const ddc w = tw_t[pos * (M / (2 * h))];
      const ddc x0 = buf[i0];
      const ddc x1 = ddc_mul(buf[i1], w);
      buf[i0] = {dd_add(x0.re, x1.re), dd_add(x0.im, x1.im)};
      buf[i1] = {dd_add(x0.re, dd_neg(x1.re)), dd_add(x0.im, dd_neg(x1.im))};
    }
    __syncthreads();
  }
}

// The stored f64 value of a double-double one: rn((hi + lo) * scale) per component.
__device__ __forceinline__ cplx dd_round(ddc x, double scale) {
  return {(x.re.hi + x.re.lo) * scale, (x.im.hi + x.im.lo) * scale};
}

// dd_fft, then the scatter into the PBS kernels' register layout: element e = (slot, lane) holds
// frequency fft512_freq(lane, slot), scaled, stored at dst(e).
template <int M, class Dst>
__device__ __forceinline__ void dd_fft_scatter(ddc* buf, const ddc* __restrict__ tw_t, double scale, Dst dst,
                                               unsigned long long* smax) {
  dd_fft<M>(buf, tw_t);
  double m2 = 0.0;
  for (int e = threadIdx.x; e < M; e += blockDim.x) {
    const cplx y = dd_round(buf[fft512_freq(e & 63, e >> 6)], scale);
    *dst(e) = y;
    m2 = fmax(m2, spec_mag2(y.re, y.im));
  }
  spec_max_commit(smax, m2);
}

// N = 1024, k = 1, l <= 3 (pbs.hip).  Block = (poly, limb), poly the index in the standard layout.
// tables: zeta[j] = exp(i pi j / N) for j < N/2 ; tw[t] = exp(-2 pi i t / (N/2)) for t < N/4
template <int LIMBS>
__global__ void __launch_bounds__(256) convert_bsk_kernel(cplx* __restrict__ dest, const uint64_t* __restrict__ src,
                                                         const ddc* __restrict__ zeta_t, const ddc* __restrict__ tw_t,
                                                         uint32_t level, unsigned long long* smax) {
  constexpr int M = 512, N = 1024;
  __shared__ ddc buf[M];
  uint64_t t = blockIdx.x;
  const uint32_t limb = next_digit(t, LIMBS);
  const uint64_t poly = t;
  const uint32_t col = next_digit(t, 2), row = next_digit(t, 2), v = next_digit(t, level);
  const uint64_t i = t;
  load_twisted<M, LIMBS>(buf, src + poly * N, 1, limb, zeta_t);
  // layout [n][limb][co][ro][q][slot][lane] (pbs.hip): slots 0..3 of group (limb, co, ro) hold
  // column co / row ro, slots 4..7 hold column 1 - co / row 1 - ro, so each wave of a pair reads
  // "own" and "other" spectra at fixed positions (the own/other layout assumes k = 1)
  const uint32_t q = level - 1 - v;
  cplx* base = dest + i * (uint64_t)(LIMBS * 4 * level * M);  // per GGSW: limbs x co x ro x levels
  dd_fft_scatter<M>(buf, tw_t, 1.0 / (double)M, [&](int e) {
    const int slot = e >> 6, lane = e & 63;
    const uint32_t co = slot < 4 ? col : 1u - col, ro = slot < 4 ? row : 1u - row;
    return base + (((uint64_t)(limb * 2 + co) * 2 + ro) * level + q) * M + slot * 64 + lane;
  }, smax);
}

// N = 2048, k = 1 (pbs2048.hip).  Block = (i, limb, col, q, row).  The parity halves
// p(u) = g[2u + par] of key polynomial g (row, col), limb `limb`, as N = 1024 negacyclic polynomials:
// folded, twisted, transformed exactly like the N = 1024 key, both spectra G_e, G_o in double-double;
// then the key at the square roots of each evaluation point, K+-[f] = (G_e[f] +- s_f G_o[f]) / 2 with
// s_f = exp(i pi (1 - 4 f) / 2048) (s_f^2 = alpha_f), correctly rounded from double-double.  Layout
// [n][limb][col][q][row][+-][slot][lane] (level v = l - 1 - q, q in digit order), scaled 1/512.
template <int LIMBS>
__global__ void __launch_bounds__(256) convert_bsk2048_kernel(cplx* __restrict__ dest, const uint64_t* __restrict__ src,
                                                             const ddc* __restrict__ zeta_t,
                                                             const ddc* __restrict__ tw_t,
                                                             const ddc* __restrict__ sroot_t, uint32_t level,
                                                             unsigned long long* smax) {
  constexpr int M = 512;
  __shared__ ddc buf[2][M];
  const uint64_t blk = blockIdx.x;
  uint64_t t = blk;
  const uint32_t row = next_digit(t, 2), q = next_digit(t, level), col = next_digit(t, 2);
  const uint32_t limb = next_digit(t, LIMBS);
  const uint64_t i = t;
  const uint32_t v = level - 1 - q;
  const uint64_t* g = src + ((i * level + v) * 4 + row * 2 + col) * 2048;  // [n][l][row][col][N]
  // as a loop: written out as two calls the kernel takes 65 VGPRs, above every kernel this file had (63)
  for (int par = 0; par < 2; ++par) load_twisted<M, LIMBS>(buf[par], g + par, 2, limb, zeta_t);
  dd_fft<M>(buf[0], tw_t);
  dd_fft<M>(buf[1], tw_t);
  const double scale = 0.5 / (double)M;
  cplx* base = dest + blk * 2 * M;
  double m2 = 0.0;
  for (int e = threadIdx.x; e < M; e += blockDim.x) {
    const int f = fft512_freq(e & 63, e >> 6);
    const ddc so = ddc_mul(buf[1][f], sroot_t[f]);
    const ddc ge = buf[0][f];
    const ddc kp{dd_add(ge.re, so.re), dd_add(ge.im, so.im)};
    const ddc km{dd_add(ge.re, dd_neg(so.re)), dd_add(ge.im, dd_neg(so.im))};
    const cplx yp = dd_round(kp, scale), ym = dd_round(km, scale);
    base[e] = yp;
    base[M + e] = ym;
    m2 = fmax(m2, fmax(spec_mag2(yp.re, yp.im), spec_mag2(ym.re, ym.im)));
  }
  spec_max_commit(smax, m2);
}

// N = 1024, k = 2 (pbs1024k2.hip).  Block = (i, limb, col, q, row), in the order of the output layout
// [n][limb][col][q][row][512] (l >= K2_MANY_MIN: level-major, [n][q][limb][col][row][512]): limb `limb`
// of key polynomial (row, col) of level v = l - 1 - q (q in digit order), folded, twisted and
// transformed like the k = 1 key.
__global__ void __launch_bounds__(256) convert_bsk1024k2_kernel(cplx* __restrict__ dest,
                                                               const uint64_t* __restrict__ src,
                                                               const ddc* __restrict__ zeta_t,
                                                               const ddc* __restrict__ tw_t, uint32_t level,
                                                               unsigned long long* smax) {
  constexpr int M = 512, N = 1024;
  __shared__ ddc buf[M];
  const uint64_t blk = blockIdx.x;
  uint64_t t = blk;
  const uint32_t row = next_digit(t, 3);
  uint32_t q, col, limb;
  if (level >= K2_MANY_MIN) {  // level-major: [n][q][limb][col][row]
    col = next_digit(t, 3), limb = next_digit(t, K2_LIMBS), q = next_digit(t, level);
  } else {
    q = next_digit(t, level), col = next_digit(t, 3), limb = next_digit(t, K2_LIMBS);
  }
  const uint64_t i = t;
  const uint32_t v = level - 1 - q;
  const uint64_t* g = src + (((i * level + v) * 3 + row) * 3 + col) * N;  // [n][l][row][col][N]
  load_twisted<M, K2_LIMBS>(buf, g, 1, limb, zeta_t);
  dd_fft_scatter<M>(buf, tw_t, 1.0 / (double)M, [&](int e) { return dest + blk * M + e; }, smax);
}

// N = 512, k = 3 / N = 256, k = 5, 6, l <= 3 (pbs_small.hip) and N = 512, k = 4, l = 1, 3 .. 5
// (pbs512k4.hip).  Block = (i, limb, cg, q, c2, row) in the order of the output layout
// [n][limb][cg][q][c2][row][N/2] (a key group: one limb, one level, GC = sm_gc(N, K1) output columns
// col = cg GC + c2): limb `limb` of key polynomial (row, col) of level v = l - 1 - q (q in digit
// order), folded, twisted by zeta_2N^j and transformed (M = N / 2 points), scaled 1 / (512 P) with
// P = 1024 / N (the kernels' unnormalised unzip and zip), element e = (slot, lane) at frequency
// fft512_freq(lane, slot).  k = 4, N = 512, l >= K4_MANY_MIN: level-major, [n][q][limb][col][row][N/2].
template <int N, int K1, int LIMBS = SM_LIMBS>
__global__ void __launch_bounds__(256) convert_bsk_small_kernel(cplx* __restrict__ dest,
                                                               const uint64_t* __restrict__ src,
                                                               const ddc* __restrict__ zeta_t,
                                                               const ddc* __restrict__ tw_t, uint32_t level,
                                                               unsigned long long* smax) {
  constexpr int M = N / 2, P = 1024 / N;
  constexpr int GC = sm_gc(N, K1), NCG = K1 / GC;
  __shared__ ddc buf[M];
  const uint64_t blk = blockIdx.x;
  uint64_t t = blk;
  const uint32_t row = next_digit(t, K1);
  uint32_t c2, q, cg, limb;
  if (N == 512 && K1 == 5 && level >= K4_MANY_MIN) {  // level-major: [n][q][limb][col][row] (GC = 1)
    c2 = 0, cg = next_digit(t, K1), limb = next_digit(t, LIMBS), q = next_digit(t, level);
  } else {
    c2 = next_digit(t, GC), q = next_digit(t, level), cg = next_digit(t, NCG), limb = next_digit(t, LIMBS);
  }
  const uint64_t i = t;
  const uint32_t col = cg * GC + c2, v = level - 1 - q;
  const uint64_t* g = src + (((i * level + v) * K1 + row) * K1 + col) * N;  // [n][l][row][col][N]
  load_twisted<M, LIMBS>(buf, g, 1, limb, zeta_t);
  dd_fft_scatter<M>(buf, tw_t, 1.0 / (512.0 * P), [&](int e) { return dest + blk * M + e; }, smax);
}

// One workgroup of 256 threads per (polynomial, limb) of the key, on a.stream; `rest`: the kernel's
// arguments after dest and src.  0, or -1 with the error recorded.
template <class... P, class... A>
static int launch_convert(void (*kernel)(P...), const ConvertArgs& a, A... rest) {
  const uint64_t blocks = (uint64_t)a.n * a.level * (a.k + 1) * (a.k + 1) * a.limbs;
  hipLaunchKernelGGL(kernel, dim3((uint32_t)blocks), dim3(256), 0, a.stream, reinterpret_cast<cplx*>(a.dest),
                     a.src_dev, rest...);
  hipError_t e = hipGetLastError();
  if (e != hipSuccess) {
    set_error("convert launch failed: %s", hipGetErrorString(e));
    return -1;
  }
  return 0;
}

struct dd_host {
  double hi, lo;
};
// dd twiddle tables from long double (64-bit mantissa): hi = rn(x), lo = rn(x - hi)
static void make_tables(uint32_t N, std::vector<ddc>& zeta, std::vector<ddc>& tw) {
  const long double PI = 3.14159265358979323846264338327950288L;
  const uint32_t M = N / 2;
  zeta.resize(M);
  tw.resize(M / 2);
  auto split = [](long double x) -> dd_host {
    double hi = (double)x;
    double lo = (double)(x - (long double)hi);
    return {hi, lo};
  };
  for (uint32_t j = 0; j < M; ++j) {
    long double ang = PI * (long double)j / (long double)N;
    dd_host c = split(cosl(ang)), s = split(sinl(ang));
    zeta[j] = {{c.hi, c.lo}, {s.hi, s.lo}};
  }
  for (uint32_t t = 0; t < M / 2; ++t) {
    long double ang = -2.0L * PI * (long double)t / (long double)M;
    dd_host c = split(cosl(ang)), s = split(sinl(ang));
    tw[t] = {{c.hi, c.lo}, {s.hi, s.lo}};
  }
}
// square roots s_f = exp(i pi (1 - 4 f) / 2048) of the N = 1024 evaluation points, f < 512
static void make_sroots(std::vector<ddc>& sr) {
  const long double PI = 3.14159265358979323846264338327950288L;
  sr.resize(512);
  for (uint32_t f = 0; f < 512; ++f) {
    const long double ang = PI * (1.0L - 4.0L * (long double)f) / 2048.0L;
    const long double c = cosl(ang), s = sinl(ang);
    const double ch = (double)c, sh = (double)s;
    sr[f] = {{ch, (double)(c - (long double)ch)}, {sh, (double)(s - (long double)sh)}};
  }
}

// A host table in stream-ordered device memory (freed by the caller after the launch).
static ddc* upload_table(const std::vector<ddc>& t, hipStream_t s) {
  ddc* d = nullptr;
  CHIP_CHECK(pool_alloc((void**)&d, t.size() * sizeof(ddc), s));
  CHIP_CHECK(hipMemcpyAsync(d, t.data(), t.size() * sizeof(ddc), hipMemcpyHostToDevice, s));
  return d;
}

int convert_bsk_launch(const ConvertArgs& a) {
  const KeyFormat f = key_format(a.k, a.N, a.level);
  if (f.kind == KeyKind::GENERIC) return convert_bsk_generic_launch(a);
  if (f.kind == KeyKind::NONE || a.limbs != f.limbs) {
    set_error("unsupported BSK conversion parameters: N=%u k=%u level=%u limbs=%u", a.N, a.k, a.level, a.limbs);
    return -2;
  }
  std::vector<ddc> zeta, tw, sr;
  make_tables(f.kind == KeyKind::SMALL ? a.N : 1024, zeta, tw);  // the others transform N = 1024 negacyclic polynomials
  ddc *dz = upload_table(zeta, a.stream), *dt = upload_table(tw, a.stream), *ds = nullptr;
  int rc;
  switch (f.kind) {
    case KeyKind::N2048:
      make_sroots(sr);
      ds = upload_table(sr, a.stream);
      rc = launch_convert(convert_bsk2048_kernel<PBS2_LIMBS>, a, dz, dt, ds, a.level, a.smax);
      break;
    case KeyKind::K2N1024: rc = launch_convert(convert_bsk1024k2_kernel, a, dz, dt, a.level, a.smax); break;
    case KeyKind::SMALL:
      rc = launch_convert(a.N == 512 && a.k == 3         ? convert_bsk_small_kernel<512, 4>
                          : a.limbs == K4_L2_LIMBS       ? convert_bsk_small_kernel<512, 5, K4_L2_LIMBS>
                          : a.N == 512                   ? convert_bsk_small_kernel<512, 5>
                          : a.k == 5                     ? convert_bsk_small_kernel<256, 6>
                                                         : convert_bsk_small_kernel<256, 7>,
                          a, dz, dt, a.level, a.smax);
      break;
    default: rc = launch_convert(convert_bsk_kernel<3>, a, dz, dt, a.level, a.smax); break;  // N1024
  }
  // the host tables must outlive the async copies: synchronise before they go out of scope
  CHIP_CHECK(hipStreamSynchronize(a.stream));
  CHIP_CHECK(hipFreeAsync(dz, a.stream));
  CHIP_CHECK(hipFreeAsync(dt, a.stream));
  if (ds) CHIP_CHECK(hipFreeAsync(ds, a.stream));
  return rc;
}

}  // namespace chip
