// kernel_util.hpp — device scaffolding shared by every fused PBS kernel (pbs.hip, pbs1024_quad.hip,
// pbs1024_hex.hip, pbs2048.hip, pbs1024k2.hip, pbs_small.hip, pbs512k4.hip) and by pbs_generic.hip /
// keyswitch.hip: the wave-group sync on LDS counters and its bounded spin, the LDS-DMA issue of a
// key-ring group, the limb rounding constants, the RESID epilogue and the step pieces
// of the N = 1024, k = 1 family and of the 16-bit limb-grid family.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include <type_traits>

#include "common.hpp"
#include "fft512.hpp"

namespace chip {

// compile-time loop: f(std::integral_constant<int, I>) for I in [B, E)
template <int B, int E, class F>
__device__ __forceinline__ void static_for(F&& f) {
  if constexpr (B < E) {
    f(std::integral_constant<int, B>{});
    static_for<B + 1, E>(f);
  }
}

// bits(v + 1.5 * 2^52) = bits(1.5 * 2^52) + round(v) for |v| < 2^51
constexpr double RND_MAGIC = 6755399441055744.0;
constexpr uint64_t RND_MAGIC_BITS = 0x4338000000000000ull;
// sum over the key limbs of the rounding constant at each limb's shift (`bits` per limb): removed
// once per recombination
constexpr uint64_t limb_magic_all(int limbs, int bits) {
  uint64_t m = 0;
  for (int li = 0; li < limbs; ++li) m += RND_MAGIC_BITS << (bits * li);
  return m;
}
// the N = 1024, k = 1 key's three balanced limbs of 22/21/21 bits: shifts 0, 22, 43
constexpr int limb_shift(int li) { return li * 21 + (li > 0 ? 1 : 0); }
constexpr uint64_t MAGIC_ALL_3 =
    (RND_MAGIC_BITS << limb_shift(0)) + (RND_MAGIC_BITS << limb_shift(1)) + (RND_MAGIC_BITS << limb_shift(2));

// Workgroup barrier (two to eight waves, every ciphertext of the workgroup): LDS writes drained,
// compiler fence, no vmcnt drain (key loads may stay in flight).
__device__ __forceinline__ void pair_barrier() { asm volatile("s_waitcnt lgkmcnt(0)\n\ts_barrier" ::: "memory"); }

// Bounded spin on an LDS counter: returns once *ctr >= target.  A wave that polls more than
// guard.spin_limit times (default 2^22 polls, far beyond any legitimate wait) stops waiting so a
// synchronisation bug cannot hang the GPU, and flags DEV_STATUS_SYNC_TIMEOUT in the device status
// word (a vector atomic): the results of that launch are then wrong, and the host reports it at
// the next synchronisation point (cuda_synchronize_device aborts, concrete_hip_device_status
// returns an error).
__device__ __forceinline__ void spin_until_ge(const uint32_t* ctr, uint32_t target, const SyncGuard& guard) {
  for (uint32_t it = 0;; ++it) {
    if (__hip_atomic_load(ctr, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP) >= target) break;
    if (it >= guard.spin_limit) {
      __hip_atomic_fetch_or(guard.status, DEV_STATUS_SYNC_TIMEOUT, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
      break;
    }
    __builtin_amdgcn_s_sleep(0);  // shortest back-off (s_sleep 1 measured -0.3 %, none -1.8 %)
  }
  asm volatile("" ::: "memory");
}
// The same wait on counters ctr[0 .. NC) at once: the NC reads are issued together per poll.
// (The cooperative kernel's grid-wide wait, pbs_generic.hip gen_coop_kernel, polls from lane 0 only
// and keeps its own loop.)
template <int NC>
__device__ __forceinline__ void spin_until_all_ge(const uint32_t* ctr, uint32_t target, const SyncGuard& guard) {
  for (uint32_t it = 0;; ++it) {
    uint32_t lo = 0xffffffffu;
#pragma unroll
    for (int o = 0; o < NC; ++o) {
      const uint32_t x = __hip_atomic_load(ctr + o, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
      lo = x < lo ? x : lo;
    }
    if (lo >= target) break;
    if (it >= guard.spin_limit) {
      __hip_atomic_fetch_or(guard.status, DEV_STATUS_SYNC_TIMEOUT, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
      break;
    }
    __builtin_amdgcn_s_sleep(0);
  }
  asm volatile("" ::: "memory");
}

// Synchronisation of the G waves that share one ciphertext, on G LDS counters f[0 .. G): wave v of
// the group publishes in f[v] how many sync points it has passed and waits until its G - 1
// partners, visited in the order v + 1, v + 2, ... (mod G), have reached the same count, so the
// other ciphertexts of the workgroup are not held up as they would be by s_barrier.
// Only LDS traffic is drained (lgkmcnt), never the key DMA: the store is relaxed, since a release
// fence would add vmcnt(0).  LDS operations are coherent across the waves of a CU, and those of
// one wave execute in issue order, which is what the split form relies on: group_signal, placed
// after this wave's reads of its partners' scratch, is seen only after those reads; group_wait,
// placed before this wave next overwrites its own scratch, waits for the partners' signals.
// group_sync is the full exchange point (my LDS writes drained, then signal and wait in one).
template <int G>
__device__ __forceinline__ int group_partner(int v, int o) {
  static_assert(G == 3 || (G & (G - 1)) == 0, "group sizes in use");
  if constexpr (G == 2) return v ^ 1;
  else if constexpr ((G & (G - 1)) == 0) return (v + o) & (G - 1);
  else return o == 1 ? (v == G - 1 ? 0 : v + 1) : (v == 0 ? G - 1 : v - 1);  // G = 3
}
template <int G>
__device__ __forceinline__ void group_signal(uint32_t* f, int v, uint32_t& cnt) {
  asm volatile("" ::: "memory");
  ++cnt;
  __hip_atomic_store(&f[v], cnt, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
}
template <int G>
__device__ __forceinline__ void group_wait(const uint32_t* f, int v, uint32_t cnt, const SyncGuard& guard) {
#pragma unroll
  for (int o = 1; o < G; ++o) spin_until_ge(&f[group_partner<G>(v, o)], cnt, guard);
  asm volatile("" ::: "memory");
}
template <int G>
__device__ __forceinline__ void group_sync(uint32_t* f, int v, uint32_t& cnt, const SyncGuard& guard) {
  asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
  ++cnt;
  __hip_atomic_store(&f[v], cnt, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
#pragma unroll
  for (int o = 1; o < G; ++o) spin_until_ge(&f[group_partner<G>(v, o)], cnt, guard);
}
// group_sync composed from the split form (two more compiler fences, which move the scheduler's
// choices): the form pbs512k4.hip and the many-level kernel of pbs1024k2.hip were tuned with
template <int G>
__device__ __forceinline__ void group_sync_composed(uint32_t* f, int v, uint32_t& cnt, const SyncGuard& guard) {
  asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
  group_signal<G>(f, v, cnt);
  group_wait<G>(f, v, cnt, guard);
}

// RESID tail of every fused kernel: this wave's largest rounding residual |x - round(x)| folded into
// *resid_out (the bits of a non-negative double order as an unsigned integer)
__device__ __forceinline__ void report_resid(double max_resid, int lane, bool active, unsigned long long* resid_out) {
  for (int off = 32; off > 0; off >>= 1) max_resid = fmax(max_resid, __shfl_xor(max_resid, off));
  if (lane == 0 && active && resid_out) atomicMax(resid_out, (unsigned long long)__double_as_longlong(max_resid));
}

// Diagnostic cycle stamps (STAMPS builds only; never in the product kernel).
__device__ __forceinline__ uint64_t stamp() {
  uint64_t t;
  __builtin_amdgcn_sched_barrier(0);
  asm volatile("s_memtime %0\n\ts_waitcnt lgkmcnt(0)" : "=s"(t)::"memory");
  __builtin_amdgcn_sched_barrier(0);
  return t;
}
constexpr int NSTAMP = 10;  // rot+decomp, fwd+xchg, mac, y-xchg, inv+recomb, ring barrier, total, steps, vmcnt, -

typedef __attribute__((address_space(3))) void* lds_ptr_t;

// LDS-DMA of this wave's GLDS 1 KB pieces of one key-ring group: piece j goes from src + 1024 j
// (16 bytes per lane, lane_b = 16 lane) to dst + 64 j.  The caller orders the ring with explicit
// vmcnt waits and workgroup barriers.
// VIA_ASM: issued from inline assembly so that the compiler does not see an LDS write: with the
// builtin it treats every window's key reads as possibly aliasing the DMA and waits for all of
// them (lgkmcnt(0)) before the first FMA; this way it counts them (lgkmcnt(4) ...): +1.1 % PBS/s
// in pbs1024_pair_kernel.  M0 (the LDS base of the piece) is set inside the statement; nothing
// else in these kernels uses M0.
// (Arguments by reference: by value, pbs512k4.hip's builtin form came out with an M0 write per
// piece, 818 instead of 524 in the file.)
template <int GLDS, bool VIA_ASM>
__device__ __forceinline__ void ring_issue(const char* const& src, cplx* const& dst, const uint32_t& lane_b) {
#pragma unroll
  for (int j = 0; j < GLDS; ++j) {
    const cplx* gp = reinterpret_cast<const cplx*>(src + j * 1024 + lane_b);
    if constexpr (VIA_ASM) {
      const uint32_t m0 = (uint32_t)(uintptr_t)(lds_ptr_t)(dst + j * 64);
#pragma clang diagnostic push
#pragma clang diagnostic ignored "-Winline-asm"
      asm volatile("s_mov_b32 m0, %1\n\tglobal_load_lds_dwordx4 %0, off" : : "v"(gp), "s"(m0) : "m0", "memory");
#pragma clang diagnostic pop
    } else {
      __builtin_amdgcn_global_load_lds(gp, (lds_ptr_t)(dst + j * 64), 16, 0, 0);
    }
  }
}

// Optimisation barrier on a register value: the value is computed here and not later (the
// compiler otherwise sinks pure arithmetic past LDS barriers into later phases, where its
// operands stay live and push the kernel past 256 VGPRs).  No instruction is emitted.
__device__ __forceinline__ void pin(uint64_t& x) { asm volatile("" : "+v"(x)); }
__device__ __forceinline__ void pin(double& x) { asm volatile("" : "+v"(x)); }

template <int N_WAIT>
__device__ __forceinline__ void wait_vmcnt() {
  static_assert(N_WAIT >= 0 && N_WAIT < 64, "vmcnt range");
  // gfx9 encoding: vmcnt[3:0] | expcnt[6:4]=7 | lgkmcnt[11:8]=15 | vmcnt_hi[15:14]
  __builtin_amdgcn_s_waitcnt((N_WAIT & 15) | (7 << 4) | (15 << 8) | ((N_WAIT >> 4) << 14));
}

// ------------------------------------------------------------------------------------
// N = 1024, k = 1 family (pbs1024_pair_kernel, pbs1024_pair_slot_kernel, pbs1024_quad_kernel,
// pbs1024_hex_kernel): the step pieces the four kernels share.  A polynomial's 1024 coefficients lie
// 16 per lane, lane t holding t + 64 m; the kernels keep the NEGATED accumulator B = -acc.
// ------------------------------------------------------------------------------------
constexpr int N1K = 1024;

// Coefficient lane + 64 m of B = -(LUT_poly * X^{-bt}), bt = ms(b) (blind_rotate_assign:
// polynomial_wrapping_monic_monomial_div); 0 for a missing ciphertext.
__device__ __forceinline__ uint64_t neg_acc_coeff(const uint64_t* lut, int poly, int lane, int m, uint32_t bt,
                                                  bool active) {
  const uint32_t src = (uint32_t)(lane + 64 * m + bt) & (2 * N1K - 1);
  const uint64_t v = active ? lut[poly * N1K + (src & (N1K - 1))] : 0ull;
  return src < N1K ? 0ull - v : v;
}

// ---- ct1 = acc * X^{at} - acc = B - X^{at} B, decomposer state per coefficient.
//      Coefficient j = lane + 64 m reads B[src & (N-1)], src = j - at mod 2N, negated when
//      src >= N; o = 8 src + 8N (mod 2^32) carries the byte offset in bits 0..12 and "src < N" in
//      bit 13, so ct1 = B + (rv ^ s) - s with s = -(bit 13 of o).
//      decomp_init(x) = (x >> nrep) + bit(nrep - 1) = (x + 2^(nrep-1)) >> nrep (a wrap of
//      x + 2^(nrep-1) past 2^64 gives state 0 instead of 2^(l logB), both decomposing to zero
//      digits); nrep >= 37 under the exactness gate, so only the high word is shifted: khi is
//      2^(nrep-1) in the high word.
__device__ __forceinline__ uint32_t rot_o0(int lane, uint32_t at) {
  return ((uint32_t)(lane - (int)at) << 3) + 8u * N1K;
}
// the rotated coefficient of slot m, from the polynomial at `base` (LDS)
__device__ __forceinline__ uint64_t rot_read(const uint64_t* base, uint32_t o0, int m) {
  return *reinterpret_cast<const uint64_t*>(reinterpret_cast<const char*>(base) + ((o0 + 512u * m) & 8191u));
}
// the rotated term of slot m: -X^{at} B at coefficient lane + 64 m, from the value rv read there.
// The kernel adds its B to it (rot_term + B: a helper that took B too fixed the order of the two
// additions, and the slot kernel's listing moved with it).
__device__ __forceinline__ uint64_t rot_term(uint64_t rv, uint32_t o0, int m) {
  const uint32_t o = o0 + 512u * m;
  const uint32_t s32 = (uint32_t)((int32_t)(o << 18) >> 31);
  const uint64_t rvs = rv ^ (((uint64_t)s32 << 32) | s32);
  return rvs + (uint64_t)(s32 & 1u);
}
// decomposer state of x = B + rot_term, a coefficient of ct1; khi = 1u << (nrep - 33)
__device__ __forceinline__ uint32_t rot_state(uint64_t x, uint32_t khi, int nrep) {
  return ((uint32_t)(x >> 32) + khi) >> (nrep - 32);
}
// B of a wave that holds it in registers, into its scratch xch64 (the rotation's first step)
__device__ __forceinline__ void acc_to_scratch(uint64_t* xch64, int lane, const uint64_t (&B)[16]) {
  lane &= 63;  // the lane's range, visible to the optimiser inside the helper as it is in the kernels
#pragma unroll
  for (int m = 0; m < 16; ++m) xch64[lane + 64 * m] = B[m];
  wave_lds_fence();
}
// Recombination of limb LR.  bits(MAGIC - v) = MAGIC_BITS - round(v): the limb's exact integers,
// negated (B = -acc), shifted into the accumulator.  The constant of all limbs is removed with limb 0
// (it must not survive into the next step's rotation: X^a * const != const).
static_assert(MAGIC_ALL_3 == RND_MAGIC_BITS + (RND_MAGIC_BITS << 22) + (RND_MAGIC_BITS << 43),
              "three limbs at shifts 0, 22, 43");
// tr, ti: the rounded parts RND_MAGIC - x
template <int LR>
__device__ __forceinline__ void limb_add(uint64_t& are, uint64_t& aim, double tr, double ti) {
  if constexpr (LR == 0) {
    are += (uint64_t)__double_as_longlong(tr) - MAGIC_ALL_3;
    aim += (uint64_t)__double_as_longlong(ti) - MAGIC_ALL_3;
  } else {
    are += (uint64_t)__double_as_longlong(tr) << limb_shift(LR);
    aim += (uint64_t)__double_as_longlong(ti) << limb_shift(LR);
  }
}
// one complex value v of the inverse's output into the accumulators of its two coefficients
template <int LR, bool RESID>
__device__ __forceinline__ void recombine_one(uint64_t& are, uint64_t& aim, const cplx& v, double& max_resid) {
  const double tr = RND_MAGIC - v.re, ti = RND_MAGIC - v.im;
  if constexpr (RESID) {
    max_resid = fmax(max_resid, fabs(v.re - (RND_MAGIC - tr)));
    max_resid = fmax(max_resid, fabs(v.im - (RND_MAGIC - ti)));
  }
  limb_add<LR>(are, aim, tr, ti);
}

// ------------------------------------------------------------------------------------
// 16-bit limb-grid family (pbs2048_quad_kernel, pbs1024k2_kernel, pbs1024k2_many_kernel,
// pbs512k4_kernel, pbs512k4_many_kernel, pbs_small_kernel): the step pieces the six kernels share.
// The key polynomial is split into LIMBS balanced limbs of LB bits (4 x 16; 5 x 13 at N = 512,
// k = 4, l = 2); a wave holds 16 coefficients per lane of the accumulator acc itself (not negated).
// ------------------------------------------------------------------------------------

// Coefficient c of LUT_poly * X^{-bt}, bt = ms(b), in the ring of size N (blind_rotate_assign:
// polynomial_wrapping_monic_monomial_div); 0 where `take` is false (a missing ciphertext, an empty
// polynomial slot, a wave without accumulator).
template <int N>
__device__ __forceinline__ uint64_t acc_coeff(const uint64_t* lut, int poly, int c, uint32_t bt, bool take) {
  const uint32_t src = (uint32_t)(c + bt) & (2 * N - 1);
  const uint64_t val = take ? lut[poly * N + (src & (N - 1))] : 0ull;
  return src < N ? val : 0ull - val;
}

// ---- ct1 = X^{at} acc - acc in the wave's own scratch: coefficient c reads acc[src & (N - 1)],
//      src = c - at mod 2N, negated when src >= N.  rot_src: the index read; rot_coeff_state: the
//      decomposer state (common.hpp decomp_init) of the coefficient from the value rv read there.
template <int N>
__device__ __forceinline__ uint32_t rot_src(int c, uint32_t at) {
  return (uint32_t)(c - (int)at) & (N - 1);
}
template <class StT, int N>
__device__ __forceinline__ StT rot_coeff_state(uint64_t rv, uint64_t a, int c, uint32_t at, int nrep) {
  const uint32_t sp = (uint32_t)(c - (int)at) & (2 * N - 1);
  return (StT)decomp_init((sp < N ? rv : 0ull - rv) - a, nrep);
}

// A digit d (logB <= 24) split exactly on the limb grid: d = lo + 2^16 hi with lo balanced 16-bit
// (|lo| <= 2^15) and |hi| <= 2^(logB-17) + 1; d - lo is a multiple of 2^16, so the shift is exact.
constexpr int SUB_BITS = 16;
__device__ __forceinline__ void sub_digit_split(int32_t d, int32_t& lo, int32_t& hi) {
  lo = ((d + (1 << (SUB_BITS - 1))) & ((1 << SUB_BITS) - 1)) - (1 << (SUB_BITS - 1));
  hi = (d - lo) >> SUB_BITS;
}

// ---- key ring: the wait ahead of window r of a step of NGRP groups, until group r has landed for
//      this wave's GLDS pieces.  steady: group r + DIST - 1 belongs to this step or a next step
//      follows, so the next DIST - 1 groups may stay in flight; else this is the tail of the last
//      step, where nothing more is issued.  The caller writes
//      steady = r + DIST - 1 < NGRP || !last_step itself: evaluated in here, without the caller's
//      short-circuit, it moves four kernels' listings.
template <int GLDS, int DIST, class R>
__device__ __forceinline__ void ring_wait(bool steady, R r, R ngrp) {
  static_assert(DIST >= 1 && DIST <= 3, "vmcnt tail cases");
  if (steady) wait_vmcnt<GLDS * (DIST - 1)>();
  else if (r + 1 == ngrp) wait_vmcnt<0>();
  else if (r + 2 == ngrp) wait_vmcnt<GLDS>();
  else wait_vmcnt<GLDS * 2>();
}

// ---- rounding and recombination of limb li.  bits(v + MAGIC) = MAGIC_BITS + round(v): the limb's
//      exact integers shifted into the accumulator at 2^{LB li}.  The constant of all limbs is
//      removed with limb 0 (it must not survive into the next step's rotation: X^a * const != const).
static_assert(limb_magic_all(4, 16) ==
                  RND_MAGIC_BITS + (RND_MAGIC_BITS << 16) + (RND_MAGIC_BITS << 32) + (RND_MAGIC_BITS << 48),
              "four 16-bit limbs");
// tr, ti: the rounded parts x + RND_MAGIC
template <int LB, int LIMBS>
__device__ __forceinline__ void grid_limb_add(int li, uint64_t& are, uint64_t& aim, double tr, double ti) {
  if (li == 0) {
    are += (uint64_t)__double_as_longlong(tr) - limb_magic_all(LIMBS, LB);
    aim += (uint64_t)__double_as_longlong(ti) - limb_magic_all(LIMBS, LB);
  } else {
    are += (uint64_t)__double_as_longlong(tr) << (LB * li);
    aim += (uint64_t)__double_as_longlong(ti) << (LB * li);
  }
}
// one complex value v of the inverse's output into the accumulators of its two coefficients
template <int LB, int LIMBS, bool RESID>
__device__ __forceinline__ void grid_recombine_one(int li, uint64_t& are, uint64_t& aim, const cplx& v,
                                                   double& max_resid) {
  const double tr = v.re + RND_MAGIC, ti = v.im + RND_MAGIC;
  if constexpr (RESID) {
    max_resid = fmax(max_resid, fabs(v.re - (tr - RND_MAGIC)));
    max_resid = fmax(max_resid, fabs(v.im - (ti - RND_MAGIC)));
  }
  grid_limb_add<LB, LIMBS>(li, are, aim, tr, ti);
}
}  // namespace chip
