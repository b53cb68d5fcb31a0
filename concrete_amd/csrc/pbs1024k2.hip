// pbs1024k2.hip — batched classic PBS for N = 1024, k = 2, l = 1 (the optimizer's 4-bit rows,
// v0-parameters: n = 801, logB = 23; bench.py --config opt4) and l = 2 at logB <= 15 (its rows at
// log norm2 >= 1: br 2/15) on CDNA4 (gfx950).
//
// Same semantics as pbs.hip (concrete-cpu c_api/bootstrap.rs:347-414 -> tfhe 0.10
// blind_rotate_assign + sample extract; restated in oracle/tfhe_oracle.c:ora_pbs) and the same
// exact arithmetic as pbs2048.hip:
//
// * Sub-digits on the limb grid.  The key polynomial g is split into 4 balanced 16-bit limbs,
//   g = sum_j 2^{16 j} g_j, and a digit d (logB <= 24) exactly into d = d_lo + 2^16 d_hi with d_lo
//   balanced 16-bit and |d_hi| <= 2^(logB-17) + 1, so
//       d g = sum_m 2^{16 m} (d_lo g_m + d_hi g_{m-1})   (mod 2^64, slots m = 0..3)
//   and each slot is one exact integer convolution sum over the three rows (certified error
//   < 1/2, oracle/pyoracle.py:gpu1024k2_error_bound).  Limb j's key serves slot j (d_lo) and slot
//   j + 1 (d_hi, carried into the next limb's windows).
// * The N = 1024 negacyclic products are pbs.hip's: one-wave 512-point folded, twisted
//   transforms in registers (fft512.hpp), key spectra in the same (lane, slot) order, scaled 1/512.
//
// Mapping: three waves per ciphertext; wave v owns GLWE polynomial v of the accumulator (16 u64
// per lane, lane t holds coefficient t + 64 m), runs the forward transforms of its own two
// sub-digit polynomials, keeps frequency slots [SB(v), SB(v+1)) of all three rows' spectra (the
// rest is read by its partners from its scratch), runs the key MAC for all three outputs on its
// slots, mails each output's slots to the owning wave and runs the four inverse transforms of its
// own output.  The slot shares are 3 / 2 / 3: a workgroup of two ciphertexts is six waves, which
// land on the four SIMDs as {0, 4}, {1, 5}, {2}, {3}, so the two SIMDs holding two waves each carry
// one 3-slot and one 2-slot wave (ciphertext 0's waves 0, 1 and ciphertext 1's waves 1, 2).
// The two ciphertexts of a workgroup share a ring of 24 KB key groups (one limb and one output
// column: three row spectra) filled by LDS-DMA, so the key crosses the L2->CU port once per
// workgroup.
#include "common.hpp"
#include "fft512.hpp"
#include "kernel_util.hpp"
#include "pbs.hpp"
#include "pbs_launch.hpp"

#include <type_traits>

namespace chip {

namespace {

// first frequency slot of wave v's share (v = 0, 1, 2; SB(3) = 8)
constexpr int K2_SB1 = 3, K2_SB2 = 5;
// Diagnostic builds only (timing; wrong results): K2D_NOBAR (no key-window barriers), K2D_NOMAC
// (no key MAC FMAs), K2D_NOINV / K2D_NOFWD (no inverse / forward transforms), K2D_NOTRI (no
// three-wave syncs).
#ifndef K2D_NOBAR
#define K2D_NOBAR 0
#endif
#ifndef K2D_NOMAC
#define K2D_NOMAC 0
#endif
#ifndef K2D_NOINV
#define K2D_NOINV 0
#endif
#ifndef K2D_NOFWD
#define K2D_NOFWD 0
#endif
#ifndef K2D_NOTRI
#define K2D_NOTRI 0
#endif
#ifndef K2D_NOROT
#define K2D_NOROT 0
#endif
#ifndef K2D_NOXRD
#define K2D_NOXRD 0
#endif
__device__ __forceinline__ int k2_slot_base(int v) { return v == 0 ? 0 : (v == 1 ? K2_SB1 : K2_SB2); }

// Sync group (kernel_util.hpp group_*<3>): the three waves of one ciphertext, tf = its counters; in
// the many-level kernel the four waves of one ciphertext (group_*<4>, counter index = role).
__device__ __forceinline__ void tri_sync(uint32_t* tf, int v, uint32_t& cnt, const SyncGuard& guard) {
  if constexpr (K2D_NOTRI) asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
  else group_sync<3>(tf, v, cnt, guard);
}
__device__ __forceinline__ void tri_wait(const uint32_t* tf, int v, uint32_t cnt, const SyncGuard& guard) {
  if constexpr (!K2D_NOTRI) group_wait<3>(tf, v, cnt, guard);
}

}  // namespace

// NQ = 1: l = 1, the two sub-digits of one digit (d_hi carried into the next slot); NQ = l = 2 (from
// l = 3 pbs1024k2_many_kernel runs one level at a time):
// whole digits (l 2^(logB-1) <= 2^15), the levels' products in the same slot (the key
// holds both levels, [n][limb][col][q][row][512], one ring group per level).
template <bool RESID, int NQ>
__global__ void __launch_bounds__(K2_CTS * 192, 1)
pbs1024k2_kernel(uint64_t* __restrict__ out, const uint64_t* __restrict__ out_idx,
                 const uint64_t* __restrict__ luts, const uint64_t* __restrict__ lut_idx,
                 const uint64_t* __restrict__ in, const uint64_t* __restrict__ in_idx,
                 const cplx* __restrict__ fbsk, uint32_t n, uint32_t base_log, uint32_t num_samples,
                 unsigned long long* __restrict__ resid_out, SyncGuard guard) {
  constexpr int N = 1024, LOG2_2N = 11, K1 = 3;
  constexpr int NW = 3 * K2_CTS;              // waves per workgroup
  constexpr bool LEVELS = NQ > 1;             // key levels per (limb, column): NQ
  constexpr int NF = LEVELS ? NQ : K2_SUBS;   // digit polynomials (sub-digits or levels) per step
  using StT = std::conditional_t<(NQ > 2), uint64_t, uint32_t>;  // decomposition state (l logB bits)
  constexpr int GROUP = K1 * 512;             // (limb, column[, level]): the three row spectra
  constexpr int NGRP = K2_LIMBS * K1 * NQ;    // ring groups per CMUX step
  constexpr int PER_I = NGRP * GROUP;         // complex values per Fourier GGSW
  constexpr int RS = K2_RING_SLOTS, DIST = K2_RING_SLOTS - 1;
  constexpr int GLDS = GROUP / 64 / NW;       // 1 KB LDS-DMA pieces per wave per group
  constexpr int XS = (int)PBS1024_XCH_SLOTS;
  constexpr int MS = 3;                       // largest slot share
  static_assert(GROUP % (64 * NW) == 0 && NGRP % RS == 0, "ring geometry");
  static_assert(XCH_SLOTS <= XS, "transpose scratch");

  extern __shared__ __attribute__((aligned(16))) char smem[];
  cplx* tbl = reinterpret_cast<cplx*>(smem);   // FFT tables (fft512.hpp)
  cplx* xch_all = tbl + FFT512_TABLE_ENTRIES;  // NW x XS: transpose scratch and mailboxes
  cplx* ring = xch_all + NW * XS;              // RS x GROUP key ring
  uint32_t* tflags = reinterpret_cast<uint32_t*>(ring + RS * GROUP);  // NW sync counters

  const int w = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  const int lane = threadIdx.x & 63;
  const int ctl = w / 3;  // ciphertext within the workgroup
  const int v = w - 3 * ctl;  // own polynomial
  uint32_t* tf = tflags + ctl * 3;  // this ciphertext's three counters
  const int sb = k2_slot_base(v);
  // slots of my share; every share has at least 2 (K2_SB1, K2_SB2), so only slot 2 is conditional
  const int ns = (v == 2 ? 8 : k2_slot_base(v + 1)) - sb;
  static_assert(K2_SB1 >= 2 && K2_SB2 - K2_SB1 >= 2 && 8 - K2_SB2 >= 2 && K2_SB1 <= 3 && K2_SB2 - K2_SB1 <= 3 &&
                    8 - K2_SB2 <= 3,
                "slot shares of 2 or 3");
  auto has = [&](int jj) __attribute__((always_inline)) { return jj < 2 || ns > 2; };
  const uint32_t s = blockIdx.x * K2_CTS + ctl;
  const bool active = s < num_samples;
  cplx* xch = xch_all + w * XS;
  uint64_t* xch64 = reinterpret_cast<uint64_t*>(xch);
  cplx* ctx = xch_all + ctl * 3 * XS;  // the three scratches of this ciphertext

  // ---- key ring: group g = (step g / NGRP, r = g % NGRP) -> slot g % RS (a constant within a
  // step: NGRP is a multiple of RS), so the refill is one wave-uniform base plus immediates.
  const cplx* key_w = fbsk + (uint64_t)w * GLDS * 64;  // this wave's pieces of every group
  cplx* ring_w = ring + w * GLDS * 64;
  const uint32_t lane_b = (uint32_t)lane * (uint32_t)sizeof(cplx);
  auto issue_group = [&](const cplx* key_step, int r) __attribute__((always_inline)) {
    ring_issue<GLDS, false>(reinterpret_cast<const char*>(key_step + r * GROUP), ring_w + (r % RS) * GROUP, lane_b);
  };
  if (n > 0) {
#pragma unroll
    for (int g = 0; g < DIST; ++g) issue_group(key_w, g);
  }

  build_fft512_tables(tbl, threadIdx.x, NW * 64);
  if (lane == 0) tflags[w] = 0u;
  uint32_t tcnt = 0;
  __syncthreads();
  const Fft512Tables T = fft512_tables_at(tbl);

  const uint64_t* lwe = in + (active ? (in_idx ? in_idx[s] : s) : 0) * (uint64_t)(n + 1);
  const uint64_t* lut = luts + (active && lut_idx ? lut_idx[s] : 0ull) * (uint64_t)(K1 * N);

  // acc_v = LUT_v * X^{-ms(b)}: lane t holds coefficients t + 64 m
  uint64_t A[16];
  {
    const uint32_t bt = active ? modswitch(lwe[n], LOG2_2N) : 0u;
#pragma unroll
    for (int m = 0; m < 16; ++m) A[m] = acc_coeff<N>(lut, v, lane + 64 * m, bt, active);
  }

  const int nrep = 64 - NQ * (int)base_log;
  const int logB = (int)base_log;
  double max_resid = 0.0;

  uint64_t a_next = active ? lwe[0] : 0ull;
  for (uint32_t i = 0; i < n; ++i) {
    const cplx* key_step = key_w + (uint64_t)i * PER_I;
    const bool last_step = i + 1 >= n;
    const uint64_t ai = a_next;
    if (i + 1 < n) a_next = active ? lwe[i + 1] : 0ull;
    const uint32_t at = modswitch(ai, LOG2_2N);
    // a zero mask element (tfhe skips it) runs on ct1 = 0: exact zeros throughout (pbs.hip)

    // ---- ct1 = X^{at} acc - acc within my own scratch (nobody else reads or writes it between
    //      the last limb's mailbox read and this step's first spectrum exchange)
    StT st[16];
    {
#pragma unroll
      for (int m = 0; m < 16; ++m) xch64[lane + 64 * m] = A[m];
      wave_lds_fence();
      uint64_t rv[16];
#pragma unroll
      for (int m = 0; m < 16; ++m) rv[m] = K2D_NOROT ? A[m] ^ at : xch64[rot_src<N>(lane + 64 * m, at)];
      __builtin_amdgcn_sched_barrier(0);
#pragma unroll
      for (int m = 0; m < 16; ++m) st[m] = rot_coeff_state<StT, N>(rv[m], A[m], lane + 64 * m, at, nrep);
      wave_lds_fence();
    }

    // ---- one level, two sub-digit polynomials, forward transforms ------------------------
    // X[row][sub][jj]: spectrum of row `row`'s sub-digit polynomial at my slot sb + jj
    cplx X[K1][NF][MS];
    int32_t dlo[16], dhi[16];
#pragma unroll
    for (int m = 0; m < (NQ <= 2 ? 16 : 0); ++m) {  // NQ > 2: each level's digits before its transform
      const int32_t d = decomp_next_t(st[m], logB);
      if constexpr (LEVELS) {
        dlo[m] = d;                           // level q = 0 (least significant first)
        dhi[m] = decomp_next_t(st[m], logB);  // level q = 1
      } else {
        sub_digit_split(d, dlo[m], dhi[m]);
      }
    }
#pragma unroll
    for (int sub = 0; sub < NF; ++sub) {
      {
        if constexpr (NQ > 2) {
#pragma unroll
          for (int m = 0; m < 16; ++m) dlo[m] = decomp_next_t(st[m], logB);  // level q = sub
        }
        cplx vv8[8];
#pragma unroll
        for (int m = 0; m < 8; ++m)
          vv8[m] = sub == 0 || NQ > 2 ? cplx{(double)dlo[m], (double)dlo[m + 8]} : cplx{(double)dhi[m], (double)dhi[m + 8]};
        cplx tw2[4], tw3[4];
        fwd_p2_tw(tw2, T, lane >> 3);
        fwd_p3_tw(tw3, T, lane);
        // the sub-0 exchange's "everyone has read my spectrum" wait, right before this
        // transform's first LDS write (the partners signalled right after their reads)
        if (!K2D_NOFWD)
          fft512_fwd_tw(vv8, xch, lane, tw2, tw3, 0, [&]() __attribute__((always_inline)) {
            if (sub > 0) tri_wait(tf, v, tcnt, guard);
          });
#pragma unroll
        for (int k2 = 0; k2 < 8; ++k2) xch[k2 * 64 + lane] = vv8[k2];
      }
      // The last sub-digit's spectra need no sync: the first key window's workgroup barrier
      // (which drains every wave's LDS writes) publishes them; they are read right after it.
      if (sub + 1 < NF) {
        tri_sync(tf, v, tcnt, guard);
#pragma unroll
        for (int row = 0; row < K1; ++row)
#pragma unroll
          for (int jj = 0; jj < MS; ++jj)
            if (has(jj)) X[row][sub][jj] = ctx[(K2D_NOXRD ? v : row) * XS + (sb + jj) * 64 + lane];
#pragma unroll
        for (int row = 0; row < K1; ++row)
#pragma unroll
          for (int jj = 0; jj < MS; ++jj) pin(X[row][sub][jj]);
        group_signal<3>(tf, v, tcnt);
      }
    }

    // ---- per limb: MAC for the three outputs on my slots, mail them, inverse of my own -----
    // Slot li of output cc = sum over rows of d_lo g_li + d_hi g_{li-1}: Yc[cc] carries the d_hi
    // part (from the previous limb's windows) into limb li's column-cc window, Yn[cc] starts
    // slot li + 1 with d_hi g_li.
    cplx Yc[K1][MS];
#pragma unroll
    for (int cc = 0; cc < K1; ++cc)
#pragma unroll
      for (int jj = 0; jj < MS; ++jj) Yc[cc][jj] = {0.0, 0.0};
    static_for<0, K2_LIMBS>([&](auto LI) __attribute__((always_inline)) {
      constexpr int li = decltype(LI)::value;
      if constexpr (!LEVELS) {
        constexpr bool HI = li + 1 < K2_LIMBS;  // d_hi g_3 lands at 2^64: vanishes
        cplx Yn[K1][MS];
#pragma unroll
        for (int cc = 0; cc < K1; ++cc)
#pragma unroll
          for (int jj = 0; jj < MS; ++jj) Yn[cc][jj] = {0.0, 0.0};
#pragma unroll
        for (int cc = 0; cc < K1; ++cc) {
          const int r = li * K1 + cc;  // group within the step
          // group r landed for this wave's pieces (the next DIST - 1 may stay in flight) ...
          ring_wait<GLDS, DIST>(r + DIST - 1 < NGRP || !last_step, r, NGRP);
          if (!K2D_NOBAR) pair_barrier();  // ... for every wave; everyone is done with group r - 1
          // refill the slot of group r - 1 with group r + DIST (RS = DIST + 1)
          if (r + DIST < NGRP) issue_group(key_step, r + DIST);
          else if (!last_step) issue_group(key_step + PER_I, r + DIST - NGRP);
          if constexpr (li == 0) {
            if (cc == 0) {  // the last sub-digit's spectra (see above)
#pragma unroll
              for (int row = 0; row < K1; ++row)
#pragma unroll
                for (int jj = 0; jj < MS; ++jj)
                  if (has(jj)) X[row][NF - 1][jj] = ctx[(K2D_NOXRD ? v : row) * XS + (sb + jj) * 64 + lane];
            }
          }
          cplx Ya[MS];
#pragma unroll
          for (int jj = 0; jj < MS; ++jj) Ya[jj] = Yc[cc][jj];
          const cplx* G = ring + (r % RS) * GROUP + sb * 64 + lane;
#pragma unroll
          for (int row = 0; row < K1; ++row) {
            cplx g[MS];
#pragma unroll
            for (int jj = 0; jj < MS; ++jj)
              if (has(jj)) g[jj] = G[row * 512 + jj * 64];
#pragma unroll
            for (int jj = 0; jj < (K2D_NOMAC ? 0 : MS); ++jj) {
              if (has(jj)) {
                cfma(Ya[jj], X[row][0][jj], g[jj]);
                if constexpr (HI) cfma(Yn[cc][jj], X[row][1][jj], g[jj]);
              }
            }
          }
          // column cc of slot li is complete: my slots straight into wave cc's mailbox.  Every
          // scratch has been idle (for writes of its owner) since this limb's first barrier, and
          // each wave only ever touches its own slots of a partner's scratch.
#pragma unroll
          for (int jj = 0; jj < MS; ++jj)
            if (has(jj)) ctx[cc * XS + (sb + jj) * 64 + lane] = Ya[jj];
#pragma unroll
          for (int jj = 0; jj < MS; ++jj) {
            pin(Ya[jj]);
            if constexpr (HI) pin(Yn[cc][jj]);
          }
        }
        if constexpr (HI) {
#pragma unroll
          for (int cc = 0; cc < K1; ++cc)
#pragma unroll
            for (int jj = 0; jj < MS; ++jj) Yc[cc][jj] = Yn[cc][jj];
        }
      } else {
        // l = 2: both levels' products land in slot li, one key window per (column, level)
#pragma unroll
        for (int cc = 0; cc < K1; ++cc) {
          cplx Ya[MS];
#pragma unroll
          for (int jj = 0; jj < MS; ++jj) Ya[jj] = {0.0, 0.0};
#pragma unroll
          for (int q = 0; q < NQ; ++q) {
            const int r = (li * K1 + cc) * NQ + q;  // group within the step
            ring_wait<GLDS, DIST>(r + DIST - 1 < NGRP || !last_step, r, NGRP);
            if (!K2D_NOBAR) pair_barrier();
            if (r + DIST < NGRP) issue_group(key_step, r + DIST);
            else if (!last_step) issue_group(key_step + PER_I, r + DIST - NGRP);
            if constexpr (li == 0) {
              if (cc == 0 && q == 0) {  // the second level's spectra (published by this barrier)
#pragma unroll
                for (int row = 0; row < K1; ++row)
#pragma unroll
                  for (int jj = 0; jj < MS; ++jj)
                    if (has(jj)) X[row][NF - 1][jj] = ctx[row * XS + (sb + jj) * 64 + lane];
              }
            }
            const cplx* G = ring + (r % RS) * GROUP + sb * 64 + lane;
#pragma unroll
            for (int row = 0; row < K1; ++row) {
              cplx g[MS];
#pragma unroll
              for (int jj = 0; jj < MS; ++jj)
                if (has(jj)) g[jj] = G[row * 512 + jj * 64];
#pragma unroll
              for (int jj = 0; jj < MS; ++jj) {
                if (has(jj)) cfma(Ya[jj], X[row][q][jj], g[jj]);
              }
            }
#pragma unroll
            for (int jj = 0; jj < MS; ++jj) pin(Ya[jj]);
          }
#pragma unroll
          for (int jj = 0; jj < MS; ++jj)
            if (has(jj)) ctx[cc * XS + (sb + jj) * 64 + lane] = Ya[jj];
        }
      }
      cplx V[8];
      tri_sync(tf, v, tcnt, guard);
#pragma unroll
      for (int k2 = 0; k2 < 8; ++k2) V[k2] = xch[k2 * 64 + lane];
      {
        cplx gi2[4];
        inv_p2_stage_tw(gi2, T, lane & 7);
        if (!K2D_NOINV) fft512_inv_tw(V, xch, T, lane, gi2, 0);
      }
#pragma unroll
      for (int m = 0; m < 8; ++m) grid_recombine_one<16, K2_LIMBS, RESID>(li, A[m], A[m + 8], V[m], max_resid);
      // materialise A here (else the inverse tail sinks into the next limb's key windows)
#pragma unroll
      for (int m = 0; m < 16; ++m) pin(A[m]);
      if constexpr (RESID) pin(max_resid);
    });
  }

  // ---- sample extract (nth = 0): mask segment c: out[c N + j] = -A_c[N - j] (j > 0), A_c[0];
  //      body out[k N] = A_k[0]
  uint64_t* o = out + (active ? (out_idx ? out_idx[s] : s) : 0) * (uint64_t)(2 * N + 1);
  if (!active) {
  } else if (v < 2) {
#pragma unroll
    for (int m = 0; m < 16; ++m) xch64[lane + 64 * m] = A[m];
    wave_lds_fence();
#pragma unroll
    for (int m = 0; m < 16; ++m) {
      const int j = lane + 64 * m;
      const uint64_t val = xch64[(N - j) & (N - 1)];
      o[v * N + j] = j == 0 ? val : 0ull - val;
    }
  } else if (lane == 0) {
    o[2 * N] = A[0];
  }

  if constexpr (RESID) report_resid(max_resid, lane, active, resid_out);
}

// Many levels (l >= K2_MANY_MIN, runtime), whole digits, one level at a time (as
// pbs512k4_many_kernel): four waves per ciphertext — the three polynomial owners and a fourth with
// no accumulator — each keeping two of the eight spectrum slots and Y[limb][column][slot] for them
// (24 accumulators, whatever l is); the key level-major, [n][q][limb][col][row][512].
template <bool RESID>
__global__ void __launch_bounds__(K2_CTS * 256, 1)
pbs1024k2_many_kernel(uint64_t* __restrict__ out, const uint64_t* __restrict__ out_idx,
                      const uint64_t* __restrict__ luts, const uint64_t* __restrict__ lut_idx,
                      const uint64_t* __restrict__ in, const uint64_t* __restrict__ in_idx,
                      const cplx* __restrict__ fbsk, uint32_t n, uint32_t level, uint32_t base_log,
                      uint32_t num_samples, unsigned long long* __restrict__ resid_out, SyncGuard guard) {
  constexpr int N = 1024, LOG2_2N = 11, K1 = 3, LIMBS = K2_LIMBS, MS = 2;
  constexpr int NW = 4 * K2_CTS;
  constexpr int GROUP = K1 * 512;           // (level, limb, column): the three row spectra
  constexpr int WPL = LIMBS * K1;           // key windows per level
  constexpr int RS = K2_RING_SLOTS, DIST = RS - 1;
  constexpr int GLDS = 4;
  constexpr int NISS = GROUP / 64 / GLDS;   // waves 0 .. NISS - 1 issue a group's pieces
  static_assert(GROUP / 64 == GLDS * NISS && NISS <= NW && WPL % RS == 0 && DIST <= 3, "ring geometry");
  constexpr int XS = (int)PBS1024_XCH_SLOTS;
  const uint32_t NGRP = (uint32_t)WPL * level;
  const uint64_t PER_I = (uint64_t)NGRP * GROUP;

  extern __shared__ __attribute__((aligned(16))) char smem[];
  cplx* tbl = reinterpret_cast<cplx*>(smem);
  cplx* xch_all = tbl + FFT512_TABLE_ENTRIES;
  cplx* ring = xch_all + 3 * K2_CTS * XS;   // (the fourth wave has no scratch)
  uint32_t* tflags = reinterpret_cast<uint32_t*>(ring + RS * GROUP);

  const int w = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  const int lane = threadIdx.x & 63;
  const int ctl = w >> 2;
  const int role = ctl == 0 ? (w & 3) : ((w + 1) & 3);  // slots 2 role, 2 role + 1
  const bool owner = role < 3;
  const int v = owner ? role : 0;           // owned polynomial
  uint32_t* tf = tflags + ctl * 4;          // this ciphertext's four counters
  const uint32_t s = blockIdx.x * K2_CTS + ctl;
  const bool active = s < num_samples;
  cplx* ctx = xch_all + ctl * 3 * XS;
  cplx* xch = ctx + v * XS;
  uint64_t* xch64 = reinterpret_cast<uint64_t*>(xch);
  cplx* myslot = ctx + 2 * role * 64 + lane;  // + jj * 64 + scratch * XS

  const bool issuer = w < NISS;
  const cplx* key_w = fbsk + (uint64_t)(issuer ? w : 0) * GLDS * 64;
  cplx* ring_w = ring + (issuer ? w : 0) * GLDS * 64;
  const uint32_t lane_b = (uint32_t)lane * (uint32_t)sizeof(cplx);
  auto issue_group = [&](const cplx* key_step, uint32_t g) __attribute__((always_inline)) {
    if (!issuer) return;
    ring_issue<GLDS, false>(reinterpret_cast<const char*>(key_step + (uint64_t)g * GROUP),
                            ring_w + (g % RS) * GROUP, lane_b);
  };
  if (n > 0) {
#pragma unroll
    for (int g = 0; g < DIST; ++g) issue_group(key_w, (uint32_t)g);
  }

  build_fft512_tables(tbl, threadIdx.x, NW * 64);
  if (lane == 0) tflags[w] = 0u;
  uint32_t tcnt = 0;
  __syncthreads();
  const Fft512Tables T = fft512_tables_at(tbl);

  const uint64_t* lwe = in + (active ? (in_idx ? in_idx[s] : s) : 0) * (uint64_t)(n + 1);
  const uint64_t* lut = luts + (active && lut_idx ? lut_idx[s] : 0ull) * (uint64_t)(K1 * N);

  // acc_v = LUT_v * X^{-ms(b)}: lane t holds coefficients t + 64 m
  uint64_t A[16];
  {
    const uint32_t bt = active ? modswitch(lwe[n], LOG2_2N) : 0u;
#pragma unroll
    for (int m = 0; m < 16; ++m) A[m] = acc_coeff<N>(lut, v, lane + 64 * m, bt, active && owner);
  }

  const int nrep = 64 - (int)level * (int)base_log;
  const int logB = (int)base_log;
  double max_resid = 0.0;

  uint64_t a_next = active && owner ? lwe[0] : 0ull;
  for (uint32_t i = 0; i < n; ++i) {
    const cplx* key_step = key_w + (uint64_t)i * PER_I;
    const bool last_step = i + 1 >= n;
    const uint64_t ai = a_next;
    if (i + 1 < n) a_next = active && owner ? lwe[i + 1] : 0ull;
    const uint32_t at = modswitch(ai, LOG2_2N);

    uint64_t st[16];
    if (owner) {
#pragma unroll
      for (int m = 0; m < 16; ++m) xch64[lane + 64 * m] = A[m];
      wave_lds_fence();
      uint64_t rv[16];
#pragma unroll
      for (int m = 0; m < 16; ++m) rv[m] = xch64[rot_src<N>(lane + 64 * m, at)];
      __builtin_amdgcn_sched_barrier(0);
#pragma unroll
      for (int m = 0; m < 16; ++m) st[m] = rot_coeff_state<uint64_t, N>(rv[m], A[m], lane + 64 * m, at, nrep);
      wave_lds_fence();
    }

    cplx Y[LIMBS][K1][MS];
#pragma unroll
    for (int li = 0; li < LIMBS; ++li)
#pragma unroll
      for (int cc = 0; cc < K1; ++cc)
#pragma unroll
        for (int jj = 0; jj < MS; ++jj) Y[li][cc][jj] = {0.0, 0.0};
#pragma unroll 1
    for (uint32_t q = 0; q < level; ++q) {
      // ---- level q: the owners' digit polynomials and forward transforms, published by the
      //      level's first key-window barrier (every wave read the previous level's spectra right
      //      after that level's first barrier, 11 windows ago)
      if (owner) {
        cplx vv[8];
        {
          int32_t d[16];
#pragma unroll
          for (int m = 0; m < 16; ++m) d[m] = decomp_next_t(st[m], logB);
#pragma unroll
          for (int m = 0; m < 8; ++m) vv[m] = {(double)d[m], (double)d[m + 8]};
        }
        cplx tw2[4], tw3[4];
        fwd_p2_tw(tw2, T, lane >> 3);
        fwd_p3_tw(tw3, T, lane);
        fft512_fwd_tw(vv, xch, lane, tw2, tw3, 0, []() __attribute__((always_inline)) {});
#pragma unroll
        for (int k2 = 0; k2 < 8; ++k2) xch[k2 * 64 + lane] = vv[k2];
      }
      cplx X[K1][MS];
#pragma unroll
      for (int wi = 0; wi < WPL; ++wi) {
        const int li = wi / K1, cc = wi % K1;
        const uint32_t r = q * (uint32_t)WPL + (uint32_t)wi;
        if (issuer) {  // ring_wait's ladder, written out: through the helper this kernel spills two more SGPRs
          if (r + DIST - 1 < NGRP || !last_step) wait_vmcnt<GLDS * (DIST - 1)>();
          else if (r + 1 == NGRP) wait_vmcnt<0>();
          else if (r + 2 == NGRP) wait_vmcnt<GLDS>();
          else wait_vmcnt<GLDS * 2>();
        }
        pair_barrier();
        if (r + DIST < NGRP || !last_step) issue_group(key_step, r + DIST);
        if (wi == 0) {
#pragma unroll
          for (int row = 0; row < K1; ++row)
#pragma unroll
            for (int jj = 0; jj < MS; ++jj) X[row][jj] = myslot[row * XS + jj * 64];
        }
        const cplx* G = ring + (wi % RS) * GROUP + 2 * role * 64 + lane;
#pragma unroll
        for (int row = 0; row < K1; ++row) {
#pragma unroll
          for (int jj = 0; jj < MS; ++jj) {
            cfma(Y[li][cc][jj], X[row][jj], G[row * 512 + jj * 64]);
          }
        }
#pragma unroll
        for (int jj = 0; jj < MS; ++jj) pin(Y[li][cc][jj]);
      }
    }

    // ---- per limb: mail my slots of the three outputs, sync, inverse, barrier ---------------
#pragma unroll
    for (int li = 0; li < LIMBS; ++li) {
#pragma unroll
      for (int cc = 0; cc < K1; ++cc)
#pragma unroll
        for (int jj = 0; jj < MS; ++jj) myslot[cc * XS + jj * 64] = Y[li][cc][jj];
      if (owner) {
        group_sync_composed<4>(tf, role, tcnt, guard);
        cplx V[8];
#pragma unroll
        for (int k2 = 0; k2 < 8; ++k2) V[k2] = xch[k2 * 64 + lane];
        {
          cplx gi2[4];
          inv_p2_stage_tw(gi2, T, lane & 7);
          fft512_inv_tw(V, xch, T, lane, gi2, 0);
        }
#pragma unroll
        for (int m = 0; m < 8; ++m) grid_recombine_one<16, K2_LIMBS, RESID>(li, A[m], A[m + 8], V[m], max_resid);
#pragma unroll
        for (int m = 0; m < 16; ++m) pin(A[m]);
      } else {
        asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
        group_signal<4>(tf, role, tcnt);
      }
      pair_barrier();  // every owner is done with its scratch
    }
  }

  uint64_t* o = out + (active ? (out_idx ? out_idx[s] : s) : 0) * (uint64_t)(2 * N + 1);
  if (!active || !owner) {
  } else if (v < 2) {
#pragma unroll
    for (int m = 0; m < 16; ++m) xch64[lane + 64 * m] = A[m];
    wave_lds_fence();
#pragma unroll
    for (int m = 0; m < 16; ++m) {
      const int j = lane + 64 * m;
      const uint64_t val = xch64[(N - j) & (N - 1)];
      o[v * N + j] = j == 0 ? val : 0ull - val;
    }
  } else if (lane == 0) {
    o[2 * N] = A[0];
  }

  if constexpr (RESID) report_resid(max_resid, lane, active, resid_out);
}

int pbs1024k2_launch(const PbsArgs& a) {
  if (!(a.N == 1024 && a.k == 2 && a.limbs == (uint32_t)K2_LIMBS && k2_ok(a.level, a.base_log)))
    return reject_params(a);
  if (a.num_samples == 0) return 0;
  return with_resid(a, [&](auto R) {
    constexpr bool RESID = decltype(R)::value;
    if (a.level >= K2_MANY_MIN)
      return launch_fused(pbs1024k2_many_kernel<RESID>, K2_CTS, K2_CTS * 256, pbs1024k2_many_lds_bytes(), a);
    if (a.level == 1) return launch_fused(pbs1024k2_kernel<RESID, 1>, K2_CTS, K2_CTS * 192, pbs1024k2_lds_bytes(), a);
    return launch_fused(pbs1024k2_kernel<RESID, 2>, K2_CTS, K2_CTS * 192, pbs1024k2_lds_bytes(), a);
  });
}

}  // namespace chip
