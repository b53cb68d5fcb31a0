// pbs.hip — batched classic programmable bootstrap for CDNA4 (gfx950).
//
// Reference semantics: concrete-cpu c_api/bootstrap.rs:347-414 -> tfhe 0.10
// programmable_bootstrap_lwe_ciphertext_mem_optimized (blind_rotate_assign + sample extract),
// restated in oracle/tfhe_oracle.c:ora_pbs.  Batched call shape: tfhe-cuda-backend
// cuda_programmable_bootstrap_lwe_ciphertext_vector_64 as invoked by the runtime
// (compiler lib/Runtime/wrappers.cpp:237-240, lib/Runtime/GPUDFG.cpp:1214-1218).
//
// Exact arithmetic: the product digit-poly x key-poly over Z_{2^64}[X]/(X^N+1) is computed
// as LIMBS exact integer negacyclic convolutions d * g_j (g = sum_j 2^{s_j} g_j, balanced
// limbs of 22/21/21 bits) evaluated with an f64 negacyclic FFT whose worst-case rounding
// error is certified < 1/2, so rounding recovers the exact integers; the
// limbs are recombined modulo 2^64.  Results are bit-identical to the schoolbook definition.
//
// Mapping (N = 1024, k = 1): two waves per ciphertext, P ciphertexts per workgroup (P = 4; 2 or 1
// for batches too small to give every CU a workgroup of 4: launch_pair).
// Wave h of a pair
//   * owns GLWE polynomial h of the accumulator (16 u64 per lane: lane t holds t + 64 m),
//   * computes the l forward transforms of its own polynomial's digits,
//   * keeps frequency slots k2 in [4h, 4h + 4) of all (k+1) l digit spectra (the other half
//     goes to its partner through LDS),
//   * runs the multiply-accumulate with the Fourier key on its half of the frequencies for
//     both output polynomials, trades the partner's half, and runs the l inverse transforms
//     of its own output polynomial.
// Each wave stays < 256 VGPRs (two waves per SIMD).  The Fourier key is streamed through a
// 3-group LDS ring (24 KB groups = three spectra of one (column, limb) slice) filled by
// LDS-DMA (global_load_lds_dwordx4) and read by all P pairs, so it crosses the L2->CU
// port once per workgroup instead of once per ciphertext.  The whole CMUX loop runs in one
// launch with the workgroup in lockstep (one raw s_barrier per key group and per half-spectrum
// exchange).
// Full batches at l = 3 run pbs1024_pair_slot_kernel (below): the same ownership, the key products
// split by frequency slot over the eight waves and the key held in registers instead of the ring.
#include <type_traits>

#include "common.hpp"
#include "fft512.hpp"
#include "kernel_util.hpp"
#include "pbs.hpp"
#include "pbs1024_plan.hpp"
#include "pbs_hex.hpp"
#include "pbs_launch.hpp"

namespace chip {

#ifndef DIAG_NOMAC
#define DIAG_NOMAC 0  // diagnostic builds only: skip the key MAC (wrong results)
#endif

// Sync group (kernel_util.hpp group_*<2>): the two waves of a pair, f = the pair's counters, h = my
// polynomial: the half-spectrum exchanges synchronise the two waves of a pair only.  DIAG_NOXBAR:
// timing-only builds without any exchange synchronisation.
#if defined(DIAG_NOXBAR)
constexpr bool XBAR = false;
#else
constexpr bool XBAR = true;
#endif
__device__ __forceinline__ void pair_signal(uint32_t* f, int h, uint32_t& cnt) {
  if constexpr (XBAR) group_signal<2>(f, h, cnt);
}
__device__ __forceinline__ void pair_wait(uint32_t* f, int h, uint32_t cnt, const SyncGuard& guard) {
  if constexpr (XBAR) group_wait<2>(f, h, cnt, guard);
}
__device__ __forceinline__ void xchg_barrier(uint32_t* f, int h, uint32_t& cnt, const SyncGuard& guard) {
  if constexpr (!XBAR) asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
  else group_sync<2>(f, h, cnt, guard);
}

template <int P, int L, bool RESID, bool STAMPS>
__global__ void __launch_bounds__(P * 128, 2)
pbs1024_pair_kernel(uint64_t* __restrict__ out, const uint64_t* __restrict__ out_idx,
                    const uint64_t* __restrict__ luts, const uint64_t* __restrict__ lut_idx,
                    const uint64_t* __restrict__ in, const uint64_t* __restrict__ in_idx,
                    const cplx* __restrict__ fbsk, uint32_t n, uint32_t base_log, uint32_t num_samples,
                    unsigned long long* __restrict__ resid_out, SyncGuard guard) {
  constexpr int K = 1, K1 = 2, N = 1024, LOG2_2N = 11, LIMBS = 3, RQ = K1 * L;
  constexpr int PER_I = K1 * LIMBS * RQ * 512;  // complex values per Fourier GGSW
  static_assert(XCH_SLOTS <= (int)PBS1024_XCH_SLOTS, "transpose scratch");
  static_assert(FFT512_TABLE_ENTRIES * sizeof(cplx) == PBS1024_TABLE_BYTES, "table bytes");
  constexpr int NW = 2 * P;                   // waves per workgroup
  constexpr int GROUP = L * 512;              // complex values per ring group (one row of a slice)
  constexpr int NGRP = K1 * K1 * LIMBS;       // ring groups per CMUX step
  constexpr int GLDS = GROUP / 64 / NW;       // 1 KB LDS-DMA pieces per wave per group
  static_assert(GROUP % (64 * NW) == 0, "group split");

  extern __shared__ __attribute__((aligned(16))) char smem[];
  cplx* tbl = reinterpret_cast<cplx*>(smem);      // FFT tables (fft512.hpp)
  cplx* xch_all = tbl + FFT512_TABLE_ENTRIES;     // NW x PBS1024_XCH_SLOTS: transpose scratch,
  cplx* ring = xch_all + NW * PBS1024_XCH_SLOTS;  // also the mailbox; 3 x GROUP key ring
  uint32_t* pflags = reinterpret_cast<uint32_t*>(ring + 3 * GROUP);  // NW pair-sync counters

  const int w = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  const int h = w & 1;  // polynomial = frequency half
  uint32_t* pf = pflags + (w - h);  // my pair's two counters
  const uint64_t hsign = (uint64_t)h << 63;  // sign mask of the k2 ^ 4 relabeling (h = 1)
  const int lane = threadIdx.x & 63;
  const uint32_t s = blockIdx.x * P + (w >> 1);
  const bool active = s < num_samples;
  cplx* xch = xch_all + w * PBS1024_XCH_SLOTS;
  uint64_t* xch64 = reinterpret_cast<uint64_t*>(xch);
  cplx* mybox = xch;                                  // the half-spectrum mailbox is the
  const cplx* partnerbox = xch_all + (w ^ 1) * PBS1024_XCH_SLOTS;   // transpose scratch, between transforms
  cplx* partnermail = xch_all + (w ^ 1) * PBS1024_XCH_SLOTS;

  // ---- key ring: group g = (step g / NGRP, limb, co, ro) -> slot g % 3 ---------------------
  // Both waves of a pair read the same group at the same time, each its own half of the slots:
  // group (li, co, ro) holds, for slots 0..3, column co / row ro and, for slots 4..7, column
  // 1 - co / row 1 - ro, i.e. "own"/"other" relative to the reading wave (bsk.hip).
  // Within a step every group index r = (li K1 + co) K1 + ro is a compile-time constant and
  // NGRP is a multiple of 3, so a group's slot (r % 3) and its offset from the step's key base
  // are constants too: the refill is one wave-uniform base plus immediates, no division.
  static_assert(NGRP % 3 == 0, "ring slot of a group must not depend on the step");
  const cplx* key_w = fbsk + (uint64_t)w * GLDS * 64;  // this wave's pieces of every group
  cplx* ring_w = ring + w * GLDS * 64;
  const uint32_t lane_b = (uint32_t)lane * (uint32_t)sizeof(cplx);  // zero-extended lane offset
  auto issue_group = [&](const cplx* key_step, int r) __attribute__((always_inline)) {
    ring_issue<GLDS, true>(reinterpret_cast<const char*>(key_step + r * GROUP), ring_w + (r % 3) * GROUP, lane_b);
  };
  if (n > 0) {
    issue_group(key_w, 0);
    issue_group(key_w, 1);
  }

  build_fft512_tables(tbl, threadIdx.x, P * 128);
  if (lane == 0) pflags[w] = 0u;
  uint32_t pcnt = 0;
  __syncthreads();
  const Fft512Tables T = fft512_tables_at(tbl);

  const uint64_t* lwe = in + (active ? (in_idx ? in_idx[s] : s) : 0) * (uint64_t)(n + 1);
  const uint64_t* lut = luts + (active && lut_idx ? lut_idx[s] : 0ull) * (uint64_t)(K1 * N);

  // acc_h = LUT_h * X^{-ms(b)}  (blind_rotate_assign: polynomial_wrapping_monic_monomial_div).
  // The wave keeps the NEGATED accumulator B = -acc_h (16 u64 per lane): the step's
  // X^a acc - acc = B - X^a B then needs no 64-bit negation, and the recombination adds the
  // rounded negated products, which the f64 rounding gives for free (MAGIC - v).
  uint64_t B[16];
  {
    const uint32_t bt = active ? modswitch(lwe[n], LOG2_2N) : 0u;
#pragma unroll
    for (int m = 0; m < 16; ++m) B[m] = neg_acc_coeff(lut, h, lane, m, bt, active);
  }

  const int nrep = 64 - L * (int)base_log;
  const int logB = (int)base_log;
  const int32_t neg_base = -(1 << logB);
  const uint32_t half_m1 = (1u << (logB - 1)) - 1u;
  double max_resid = 0.0;
  // diagnostic stamps (STAMPS builds only): 0 rotation, 1 forward + exchange, 2 products, 8 key
  // landed (vmcnt), 5 barrier wait, 3 Y exchange, 4 inverse + recombination, 6 total, 7 work steps
  uint64_t acc_t[NSTAMP] = {};
  uint64_t t_begin = 0, tp = 0;
  auto lap = [&](int k) __attribute__((always_inline)) {
    if constexpr (STAMPS) {
      const uint64_t t = stamp();
      acc_t[k] += t - tp;
      tp = t;
    }
  };
  if constexpr (STAMPS) t_begin = stamp();

  // forward pass-3 twiddles of my lane: constant for the whole kernel, kept in registers
  cplx tw3[4];
  fwd_p3_tw(tw3, T, lane);

  uint64_t a_next = active ? lwe[0] : 0ull;
  for (uint32_t i = 0; i < n; ++i) {
    const cplx* key_step = key_w + (uint64_t)i * PER_I;
    const uint64_t ai = a_next;
    if (i + 1 < n) a_next = active ? lwe[i + 1] : 0ull;

    const uint32_t at = modswitch(ai, LOG2_2N);
    // tfhe skips a zero mask element (and at == 0 changes nothing): the step still runs, on
    // ct1 = X^0 acc - acc = 0, whose digits, spectra and products are exact zeros, so the
    // recombination adds exactly 0 (the limb constants cancel).  Running every step keeps the
    // compiler from hoisting undefined values of skipped-step arrays out of the loop, where
    // they pinned ~110 VGPRs.
    if constexpr (STAMPS) {
      tp = stamp();
      acc_t[7] += ai != 0ull && at != 0u;
    }

    // ---- own polynomial: ct1 = B - X^{at} B and the decomposer state per coefficient (the pieces and
    //      their explanation: kernel_util.hpp)
    uint32_t st[16];
    {
      acc_to_scratch(xch64, lane, B);
      const uint32_t o0 = rot_o0(lane, at), khi = 1u << (nrep - 33);
      // all 16 reads in flight at once (left to itself the scheduler issues them four at a time,
      // one LDS round trip each)
      uint64_t rv[16];
#pragma unroll
      for (int m = 0; m < 16; ++m) rv[m] = rot_read(xch64, o0, m);
      __builtin_amdgcn_sched_barrier(0);
#pragma unroll
      for (int m = 0; m < 16; ++m) st[m] = rot_state(rot_term(rv[m], o0, m) + B[m], khi, nrep);
      wave_lds_fence();
    }
    lap(0);

    // ---- forward transforms; keep my half of the slots, mail the other half -------------
    // Xo[q][j] / Xp[q][j]: spectrum of my own / my partner's digit polynomial (level q) at
    // frequency slot 4h + j.  The wave owning the upper half (h = 1) emits its spectrum in slot
    // order k2 ^ 4, so every wave keeps v[0..3] and mails v[4..7]: no h-dependent registers.
    cplx Xo[L][4], Xp[L][4];
    // levels are traded in batches of up to XB (one mailbox of 4 KB per level, <= 2): the
    // mailed halves of a batch wait in registers until its last transform is done
    constexpr int XB = 2;
#pragma unroll
    for (int q0 = 0; q0 < L; q0 += XB) {
      const int nq = (q0 + XB <= L) ? XB : L - q0;
      cplx out[XB][4];
      {
#pragma unroll
        for (int t = 0; t < XB; ++t) {
          if (t < nq) {
            // digits of level l - q (the decomposition iterator yields the least significant first)
            cplx v[8];
            int32_t d[16];
#pragma unroll
            for (int m = 0; m < 16; ++m)
              d[m] = decomp_level32(st[m], (uint32_t)((q0 + t) * logB), logB, half_m1, neg_base, q0 + t + 1 < L);
#pragma unroll
            for (int m = 0; m < 8; ++m) v[m] = {(double)d[m], (double)d[m + 8]};
            // the first transform after a mailbox exchange overwrites my scratch: my partner
            // must have read the mailbox (it signals right after its reads)
            cplx tw2[4];
            fwd_p2_tw(tw2, T, lane >> 3);
            // issued here, ahead of pass 1 and the register transpose that hide their latency
            // (left alone the scheduler sinks each read to its butterfly stage, one exposed LDS
            // round trip per stage)
            __builtin_amdgcn_sched_barrier(0);
            fft512_fwd_tw(v, xch, lane, tw2, tw3, hsign, [&]() __attribute__((always_inline)) {
              if (q0 > 0 && t == 0) pair_wait(pf, h, pcnt, guard);
            });
#pragma unroll
            for (int j = 0; j < 4; ++j) {
              Xo[q0 + t][j] = v[j];
              out[t][j] = v[4 + j];
            }
          }
        }
#pragma unroll
        for (int t = 0; t < XB; ++t)
          if (t < nq)
#pragma unroll
            for (int j = 0; j < 4; ++j) mybox[(t * 4 + j) * 64 + lane] = out[t][j];
      }
      // The last batch's halves need no pair sync: the first key window's workgroup barrier
      // (which drains every wave's LDS writes) publishes them, and they are first used in the
      // second window (row 1); they are read right after that barrier.
      const bool last_batch = q0 + XB >= L;
      if (!last_batch) {
        xchg_barrier(pf, h, pcnt, guard);
#pragma unroll
        for (int t = 0; t < XB; ++t)
          if (t < nq)
#pragma unroll
            for (int j = 0; j < 4; ++j) Xp[q0 + t][j] = partnerbox[(t * 4 + j) * 64 + lane];
      }
      // materialise this batch's spectra here (else its transforms sink into the key windows)
#pragma unroll
      for (int t = 0; t < XB; ++t)
        if (t < nq)
#pragma unroll
          for (int j = 0; j < 4; ++j) pin(Xo[q0 + t][j]);
      // my partner's mailbox has been read: signal it (it waits before its next transform writes
      // its scratch).  After the last batch the scratch is next written behind the key windows'
      // workgroup barriers.
      if (q0 + XB < L) pair_signal(pf, h, pcnt);
    }
    lap(1);

    // ---- per limb: MAC for both output polynomials on my half (key from the LDS ring),
    //      trade halves through the mailbox, inverse transform of my polynomial. ------------
    static_for<0, LIMBS>([&](auto LI) __attribute__((always_inline)) {
      constexpr int li = decltype(LI)::value;
      cplx Ymine[4];
      // co / ro: my own (0) or my partner's (1) output polynomial / input row; group
      // (li, co, ro) holds exactly those spectra for both halves (layout: bsk.hip)
#pragma unroll
      for (int co = 0; co < K1; ++co) {
        cplx Y[4];  // set by the first product of window ro = 0 (no zeroing)
        if constexpr (DIAG_NOMAC) {
#pragma unroll
          for (int j = 0; j < 4; ++j) Y[j] = {0.0, 0.0};
        }
#pragma unroll
        for (int ro = 0; ro < K1; ++ro) {
          const int r = (li * K1 + co) * K1 + ro;  // group within the step (constant)
          const bool last_step = i + 1 >= n;
          lap(2);
          // group g landed for this wave's pieces (group g + 1 may stay in flight) ...
          if (r + 1 < NGRP || !last_step) wait_vmcnt<GLDS>();
          else wait_vmcnt<0>();
          lap(8);
          // ... and for every wave's pieces; everyone is also done with group g - 1
#ifndef DIAG_NOBAR
          pair_barrier();
#endif
          lap(5);
          // refill the slot of group g - 1 with group g + 2, right after the barrier (the DMA
          // needs the lead time: issued after the window's reads or FMAs it measured slower)
#ifndef DIAG_NODMA
          if (r + 2 < NGRP) issue_group(key_step, r + 2);
          else if (!last_step) issue_group(key_step + PER_I, r + 2 - NGRP);
#endif
          if constexpr (li == 0) {
            if (co == 0 && ro == 0) {
              constexpr int QL = (L - 1) / XB * XB;  // first level of the last batch
#pragma unroll
              for (int q = QL; q < L; ++q)
#pragma unroll
                for (int j = 0; j < 4; ++j) Xp[q][j] = partnerbox[((q - QL) * 4 + j) * 64 + lane];
            }
          }
          const cplx* G = ring + (r % 3) * GROUP + (4 * h) * 64 + lane;
          // all key values of the window first, then the FMAs
          cplx gv[L][4];
#pragma unroll
          for (int q = 0; q < L; ++q)
#pragma unroll
            for (int j = 0; j < 4; ++j) gv[q][j] = G[(q * 8 + j) * 64];
#pragma unroll
          for (int q = 0; q < (DIAG_NOMAC ? 0 : L); ++q) {
#pragma unroll
            for (int j = 0; j < 4; ++j) {
              const cplx x = ro == 0 ? Xo[q][j] : Xp[q][j];
              if (ro == 0 && q == 0) {  // fma(a, b, 0) == a * b: same bits as accumulating from 0
                Y[j].re = __builtin_fma(x.re, gv[q][j].re, -x.im * gv[q][j].im);
                Y[j].im = __builtin_fma(x.re, gv[q][j].im, x.im * gv[q][j].re);
              } else {
                Y[j].re = __builtin_fma(x.re, gv[q][j].re, __builtin_fma(-x.im, gv[q][j].im, Y[j].re));
                Y[j].im = __builtin_fma(x.re, gv[q][j].im, __builtin_fma(x.im, gv[q][j].re, Y[j].im));
              }
            }
          }
          // this window's products are done here, not sunk past the next window's barrier
#pragma unroll
          for (int j = 0; j < 4; ++j) pin(Y[j]);
        }
        if (co == 0) {
#pragma unroll
          for (int j = 0; j < 4; ++j) Ymine[j] = Y[j];
        } else {
          // straight into my partner's mailbox (its scratch has been idle since the key
          // windows' workgroup barriers), so no "partner has read" sync is needed afterwards
#pragma unroll
          for (int j = 0; j < 4; ++j) partnermail[j * 64 + lane] = Y[j];
        }
      }
      lap(2);
      xchg_barrier(pf, h, pcnt, guard);
      // my output polynomial's spectrum, slots in order k2 ^ 4h (undone by the inverse pass 1)
      cplx vp[8];
#pragma unroll
      for (int j = 0; j < 4; ++j) {
        vp[j] = Ymine[j];
        vp[4 + j] = mybox[j * 64 + lane];
      }
      // no second sync: the only writes into my scratch by my partner are these Y mailboxes,
      // one per limb, always behind key-window workgroup barriers (the forward exchange only
      // reads the partner's scratch, under its own two syncs)
      lap(3);
      cplx gi2[4];  // inverse pass-2 stage twiddles, read ahead of the transpose
      inv_p2_stage_tw(gi2, T, lane & 7);
      fft512_inv_tw(vp, xch, T, lane, gi2, hsign);
#pragma unroll
      for (int m = 0; m < 8; ++m) recombine_one<li, RESID>(B[m], B[m + 8], vp[m], max_resid);
      // materialise B here (else the inverse tail sinks into the next limb's key windows)
#pragma unroll
      for (int m = 0; m < 16; ++m) pin(B[m]);
      if constexpr (RESID) pin(max_resid);
      lap(4);
    });
  }

  if constexpr (STAMPS) {
    acc_t[6] = stamp() - t_begin;
    if (lane == 0 && resid_out) {
      unsigned long long* dst = resid_out + ((uint64_t)blockIdx.x * NW + w) * NSTAMP;
      for (int q = 0; q < NSTAMP; ++q) dst[q] = acc_t[q];
    }
  }

  // ---- sample extract (nth = 0) of acc = -B: out[j] = -acc_0[N - j] (j > 0), acc_0[0]; body acc_1[0]
  uint64_t* o = out + (active ? (out_idx ? out_idx[s] : s) : 0) * (uint64_t)(K * N + 1);
  if (!active) {
  } else if (h == 0) {
    // acc = -B
#pragma unroll
    for (int m = 0; m < 16; ++m) xch64[lane + 64 * m] = B[m];
    wave_lds_fence();
#pragma unroll
    for (int m = 0; m < 16; ++m) {
      const int j = lane + 64 * m;
      const uint64_t v = xch64[(N - j) & (N - 1)];
      o[j] = j == 0 ? 0ull - v : v;
    }
  } else if (lane == 0) {
    o[K * N] = 0ull - B[0];
  }

  if constexpr (RESID && !STAMPS) report_resid(max_resid, lane, active, resid_out);
}

// ------------------------------------------------------------------------------------
// pbs1024_pair_slot_kernel (l = 3, 4 ciphertexts per workgroup): the pair kernel with the key
// shared in registers instead of through the LDS ring.
//
// Wave w = 2 ct + h owns polynomial h of ciphertext ct exactly as above (negated accumulator,
// rotation, decomposition, the three forward and three inverse transforms, recombination, sample
// extract), with fft512's natural slot order in every wave (no k2 ^ 4 relabeling).  Only the key
// products are split differently: fft512 leaves 8 frequency slots per lane and the workgroup has 8
// waves, so wave w takes slot k2 = w of all four ciphertexts, both input rows and both output
// polynomials.  A key value then serves four ciphertexts from one register: it is loaded straight
// from L2 with plain 16-byte-per-lane global loads (36 per wave and step, the bytes the ring's DMA
// moved) — no ring, no LDS-DMA, no key-window barriers.
//
// Key addressing (bsk.hip): group (limb, co, ro) holds at slot p < 4 column co / row ro and at
// slot p >= 4 column 1 - co / row 1 - ro, so wave w reads (column c, row r) of its slot from group
// (limb, c ^ f, r ^ f), f = (w >= 4): group index 2 c + r for f = 0, 3 - (2 c + r) for f = 1.
// A step's 36 values are taken in the order t = (limb, c, level q, r) through a ring of
// SLOT_PF registers: value t + SLOT_PF is requested when value t has been used.
//
// Exchanges go through one 8 KB mailbox per wave (next to its transpose scratch):
//   forward:             levels 0 and 1 together — level 0 waits in registers during the second
//                        transform, then v[0..7] -> own mailbox and level 1 -> own transpose
//                        scratch (idle between transforms) | workgroup barrier | every wave reads
//                        its slot from the 8 mailboxes and 8 scratches; the third transform, with
//                        the first window's level-0/1 products (64 of its 96 FMAs) behind the
//                        writes and reads of its LDS transpose; level 2 through
//                        the mailbox alone | workgroup barrier | reads
//   products, per limb:  Y[ct][co] -> mailbox of wave (ct, co) at position w | workgroup barrier |
//                        the wave reads its 8 slots; limb li + 1's first product window; inverse
//                        and recombination of limb li
// 5 workgroup barriers per step.  A mailbox (or published scratch) is written again only once
// every wave has issued the reads of the previous exchange: each wave adds 1 to one LDS counter
// after its reads (LDS operations of a wave execute in issue order) and writers wait for
// 8 x (exchanges so far) with spin_until_ge; a transform or a product window lies between, so the
// first poll normally passes.  (A step's first exchange needs no wait: the last readers of a
// mailbox were its owner, and the scratch was released before the third transform.)
// ------------------------------------------------------------------------------------
#ifndef SLOT_PF
#define SLOT_PF 6  // key values in flight per wave (a divisor of 36; 6 = one (limb, output) window)
#endif
// The schedule is the one stage-by-stage measurement kept (DESIGN.md §4.16,
// profiles/r11_slot/variants.json): the kernel sits at 256 VGPRs, and a stage that moves the
// register allocation moves the time by more than the work it saves or hides.
// tan(pi m / 16), m = 0..7 (correctly rounded): psi^m = psi_pow(m).re * (1 + i psi_tan(m))
__device__ __forceinline__ double psi_tan(int m) {
  constexpr double TAN[8] = {0.0,
                             0x1.975f5e0553158p-3,
                             0x1.a827999fcef32p-2,
                             0x1.561b82ab7f990p-1,
                             1.0,
                             0x1.7f218e25a7461p+0,
                             0x1.3504f333f9de6p+1,
                             0x1.41bfee2424771p+2};
  return TAN[m];
}
// the order of the stages' pieces as written, kept against the instruction scheduler
__device__ __forceinline__ void slot_order() { __builtin_amdgcn_sched_barrier(0); }
constexpr int SLOT_MBOX = 512;// complex values per mailbox: 8 slots x 64 lanes
constexpr size_t pbs1024_pair_slot_lds_bytes() {
  return PBS1024_TABLE_BYTES + 2 * (size_t)PBS_PAIRS * (PBS1024_XCH_SLOTS + SLOT_MBOX) * 16 + 16;  // + the counter
}

__device__ __forceinline__ void slot_signal(uint32_t* ctr, int lane, uint32_t& cnt) {
  asm volatile("" ::: "memory");
  ++cnt;
  if (lane == 0) __hip_atomic_fetch_add(ctr, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
}

// ---- The step's integer pieces (kernel_util.hpp: rot_term / rot_state, decomp_level32, limb_add)
//      with the decomposition base fixed at compile time (BL = base_log, L levels, L BL <= 27).
//      Every shift, field offset and constant is an immediate, and the sequences are shorter ones
//      that keep every digit and every accumulator word ("the integer path").
__device__ __forceinline__ void pin(uint32_t& x) { asm volatile("" : "+v"(x)); }
// The decomposer works on the UNSHIFTED word W = high word of ct1 + 2^(nrep-1), nrep = 64 - L BL:
// the state of decomp_level32 is W >> (nrep - 32), so level q's field lies at 32 - (L - q) BL,
// the top field ends at bit 31 and the bits below the first field are never read.
// rot_word: W of a slot from its o = o0 + 512 m (rot_term), the value rv read at the rotated place
// and the wave's own b.  With s = -(src < N) as a 64-bit mask the negation is (rv ^ s) - s: no
// separate carry word.
template <int NREP>
__device__ __forceinline__ uint32_t rot_word(uint64_t rv, uint32_t o, uint64_t b) {
  static_assert(NREP > 32 && NREP < 64, "only the high word is decomposed");
  const uint32_t s32 = (uint32_t)__builtin_amdgcn_sbfe((int32_t)o, 13u, 1u);
  const uint64_t s = ((uint64_t)s32 << 32) | s32;
  return (uint32_t)((((rv ^ s) - s) + b) >> 32) + (1u << (NREP - 33));
}
// Digit of level q (decomp_level32's recurrence and tie rule) from W, as the f64 the transform
// takes; W takes the carry.  With tc = top + B/2 - 1 added at the field's place, the field becomes
// res + tc - B carry and the bits above it take the carry: the digit res - B carry is the new field
// minus tc, and the new word is the next level's (its own field is not read again).  Above the
// last level's field there is no tie bit (the state is below 2^(L BL + 1)): its digit is
// res - B [res > B/2], which is minus the top field of 2^off - 1 - W taken signed (the negation
// goes into the transform's first operands).
template <int BL, int L>
__device__ __forceinline__ double decomp_word_digit(uint32_t& W, int q) {
  static_assert(BL >= 1 && L * BL <= 27, "the exact range of the N = 1024 kernels");
  const uint32_t off = 32u - (uint32_t)((L - q) * BL);
  if (q + 1 == L) return -(double)((int32_t)(((1u << off) - 1u) - W) >> off);
  // the tie bit: the next level's top bit, <= bit 31 since q + 2 <= L
  const uint32_t tc = __builtin_amdgcn_ubfe(W, off + 2u * BL - 1u, 1u) + ((1u << (BL - 1)) - 1u);
  W += tc << off;
  return (double)((int32_t)__builtin_amdgcn_ubfe(W, off, (uint32_t)BL) - (int32_t)tc);
}
// Recombination: limb 0's rounding constant (the only one of the three whose bits stay below 2^64:
// MAGIC_ALL_3 == RND_MAGIC_BITS, high word only) is not subtracted per coefficient but cancelled
// by limb 2's own rounding constant, RND_MAGIC + RND2_OFS: limb 2 enters at 2^43, i.e. its low
// word at bit 11 of the high word, and RND2_OFS << 11 == -(RND_MAGIC_BITS >> 32) mod 2^32.  Both
// constants are even multiples of the unit in the last place, so every rounding falls as before.
static_assert(MAGIC_ALL_3 == RND_MAGIC_BITS && (uint32_t)RND_MAGIC_BITS == 0u, "limbs 1 and 2 shift their constant out");
constexpr uint32_t RND2_OFS = (0u - (uint32_t)(RND_MAGIC_BITS >> 32)) >> (limb_shift(2) - 32);
static_assert((uint32_t)(RND2_OFS << (limb_shift(2) - 32)) + (uint32_t)(RND_MAGIC_BITS >> 32) == 0u && RND2_OFS % 2 == 0,
              "limb 2's constant removes limb 0's");
template <int LR>
constexpr double fixed_rnd_magic() { return LR == 2 ? RND_MAGIC + (double)RND2_OFS : RND_MAGIC; }
// tr, ti: the rounded parts fixed_rnd_magic<LR>() - x; limb 2 touches the high word alone (one
// 32-bit shift-add, pinned: left to itself the compiler widens it back to a 64-bit add)
__device__ __forceinline__ void hi_word_shl_add(uint64_t& a, uint64_t bits, int sh) {
  uint32_t hi = (uint32_t)(a >> 32) + ((uint32_t)bits << sh);
  pin(hi);
  a = (uint64_t)(uint32_t)a | ((uint64_t)hi << 32);
}
template <int LR>
__device__ __forceinline__ void fixed_limb_add(uint64_t& are, uint64_t& aim, double tr, double ti) {
  const uint64_t br = (uint64_t)__double_as_longlong(tr), bi = (uint64_t)__double_as_longlong(ti);
  if constexpr (LR == 0) {
    are += br, aim += bi;
  } else if constexpr (LR == 1) {
    are += br << limb_shift(1), aim += bi << limb_shift(1);
  } else {
    hi_word_shl_add(are, br, limb_shift(2) - 32);
    hi_word_shl_add(aim, bi, limb_shift(2) - 32);
  }
}

// BL: base_log fixed at compile time (the metric's 7), or 0 for a base read at run time.  With BL
// the rotation, the decomposition and the recombination take the forms above (rot_word,
// decomp_word_digit, fixed_limb_add); BL = 0 is the code as it was.
template <int BL, bool RESID, bool STAMPS>
__global__ void __launch_bounds__(PBS_PAIRS * 128, 2)
pbs1024_pair_slot_kernel(uint64_t* __restrict__ out, const uint64_t* __restrict__ out_idx,
                         const uint64_t* __restrict__ luts, const uint64_t* __restrict__ lut_idx,
                         const uint64_t* __restrict__ in, const uint64_t* __restrict__ in_idx,
                         const cplx* __restrict__ fbsk, uint32_t n, uint32_t base_log, uint32_t num_samples,
                         unsigned long long* __restrict__ resid_out, SyncGuard guard) {
  constexpr int K = 1, K1 = 2, N = 1024, LOG2_2N = 11, LIMBS = 3, L = 3, P = PBS_PAIRS, NW = 2 * P;
  constexpr int GROUP = L * 512;                  // one (limb, co, ro) group: the L level spectra
  constexpr int PER_I = K1 * K1 * LIMBS * GROUP;  // complex values per Fourier GGSW
  constexpr int NKEY = LIMBS * K1 * K1 * L;       // key values per wave and step
  constexpr int PF = SLOT_PF;
  constexpr int XS = (int)PBS1024_XCH_SLOTS, MB = SLOT_MBOX;
  static_assert(NW == 8, "one frequency slot per wave");
  static_assert(NKEY % PF == 0, "a key value's register must not depend on the step");
  static_assert(XCH_SLOTS <= XS, "transpose scratch");

  extern __shared__ __attribute__((aligned(16))) char smem[];
  cplx* tbl = reinterpret_cast<cplx*>(smem);                      // FFT tables (fft512.hpp)
  cplx* xch_all = tbl + FFT512_TABLE_ENTRIES;                     // NW transpose scratches
  cplx* mbox_all = xch_all + NW * XS;                             // NW mailboxes
  uint32_t* ctr = reinterpret_cast<uint32_t*>(mbox_all + NW * MB);  // reads-issued counter

  const int w = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  const int h = w & 1;  // polynomial
  const int lane = threadIdx.x & 63;
  const uint32_t s = blockIdx.x * P + (w >> 1);
  const bool active = s < num_samples;
  cplx* xch = xch_all + w * XS;
  uint64_t* xch64 = reinterpret_cast<uint64_t*>(xch);
  cplx* mybox = mbox_all + w * MB + lane;             // + k2 * 64
  cplx* slotbox = mbox_all + w * 64 + lane;           // + u * MB: slot w of wave u's mailbox

  // ---- key value t of a step (t = (limb K1 + c) K1 L + e, e in window order), for this wave's slot
  const bool flip = w >= 4;
  const cplx* key_w = fbsk + (w * 64 + (flip ? 3 * GROUP : 0));
  const int gstride = flip ? -GROUP : GROUP;
  auto key_load = [&](const cplx* key_step, int t) __attribute__((always_inline)) {
    const int li = t / (K1 * K1 * L), co = t / (K1 * L) % K1, e = t % (K1 * L);
    const int ro = e % K1, q = e / K1, cr = co * K1 + ro;
    return (key_step + (li * K1 * K1 * GROUP + q * 512) + cr * gstride)[lane];
  };
  cplx g[PF] = {};
  if (n > 0) {
#pragma unroll
    for (int t = 0; t < PF; ++t) g[t] = key_load(key_w, t);
  }

  build_fft512_tables(tbl, threadIdx.x, P * 128);
  if (threadIdx.x == 0) *ctr = 0u;
  uint32_t rcnt = 0;  // exchanges whose reads this wave has issued
  __syncthreads();
  const Fft512Tables T = fft512_tables_at(tbl);

  const uint64_t* lwe = in + (active ? (in_idx ? in_idx[s] : s) : 0) * (uint64_t)(n + 1);
  const uint64_t* lut = luts + (active && lut_idx ? lut_idx[s] : 0ull) * (uint64_t)(K1 * N);

  // B = -acc_h, acc_h = LUT_h * X^{-ms(b)} (pbs1024_pair_kernel).  A wave of a missing ciphertext
  // keeps B = 0 and still runs every barrier, counter and slot product of the others.
  uint64_t B[16];
  {
    const uint32_t bt = active ? modswitch(lwe[n], LOG2_2N) : 0u;
#pragma unroll
    for (int m = 0; m < 16; ++m) B[m] = neg_acc_coeff(lut, h, lane, m, bt, active);
  }

  const int logB = BL ? BL : (int)base_log;
  const int nrep = 64 - L * logB;
  const int32_t neg_base = -(1 << logB);
  const uint32_t half_m1 = (1u << (logB - 1)) - 1u;
  double max_resid = 0.0;
  // diagnostic stamps (STAMPS builds only): 0 rotation, 1 forward + exchange, 2 products,
  // 5 barrier wait, 3 Y exchange, 4 inverse + recombination, 6 total, 7 work steps
  uint64_t acc_t[NSTAMP] = {};
  uint64_t t_begin = 0, tp = 0;
  auto lap = [&](int k) __attribute__((always_inline)) {
    if constexpr (STAMPS) {
      const uint64_t t = stamp();
      acc_t[k] += t - tp;
      tp = t;
    }
  };
  if constexpr (STAMPS) t_begin = stamp();

  cplx tw3[4];  // forward pass-3 twiddles of my lane, in registers for the whole kernel
  fwd_p3_tw(tw3, T, lane);

  uint64_t a_next = active && n > 0 ? lwe[0] : 0ull;
  for (uint32_t i = 0; i < n; ++i) {
    const cplx* key_step = key_w + (uint64_t)i * PER_I;
    const cplx* key_next = i + 1 < n ? key_step + PER_I : key_step;  // past the last step: re-read (unused)
    const uint64_t ai = a_next;
    if (i + 1 < n) a_next = active ? lwe[i + 1] : 0ull;
    const uint32_t at = modswitch(ai, LOG2_2N);
    if constexpr (STAMPS) {
      tp = stamp();
      acc_t[7] += ai != 0ull && at != 0u;
    }

    // ---- ct1 = B - X^{at} B and the decomposer state (pbs1024_pair_kernel); with a fixed base the
    //      unshifted word that holds it (rot_word)
    uint32_t st[16];
    {
      acc_to_scratch(xch64, lane, B);
      const uint32_t o0 = rot_o0(lane, at), khi = 1u << (nrep - 33);
      // with a fixed base: one sum o0 + 512 m per slot, for the read's address and for the sign of
      // the rotated term (pinned: the compiler otherwise forms the sign from a second sum)
      uint32_t om[16];
#pragma unroll
      for (int m = 0; m < 16; ++m) {
        om[m] = o0 + 512u * m;
        if constexpr (BL != 0) pin(om[m]);
      }
      // all 16 reads in flight at once (left to itself the scheduler issues them four at a time,
      // one LDS round trip each)
      uint64_t rv[16];
#pragma unroll
      for (int m = 0; m < 16; ++m) rv[m] = BL != 0 ? rot_read(xch64, om[m], 0) : rot_read(xch64, o0, m);
      __builtin_amdgcn_sched_barrier(0);
#pragma unroll
      for (int m = 0; m < 16; ++m) {
        if constexpr (BL != 0) st[m] = rot_word<64 - L * BL>(rv[m], om[m], B[m]);
        else st[m] = rot_state(rot_term(rv[m], o0, m) + B[m], khi, nrep);
      }
      wave_lds_fence();
    }
    lap(0);

    // ---- forward transforms of my polynomial, one level at a time; X[q][u]: slot w of the
    //      level-q spectrum of wave u (ciphertext u / 2, row u % 2)
    cplx X[L][NW];
    const int hi = lane >> 3, lo = lane & 7;
    // products e0 <= e < e1 of one window (output co of limb li for the 4 ciphertexts), in
    // level-major (q, ro) order, which needs the last forward level's spectra only in the last
    // third of a window.  Y is set by product 0 (no zeroing).
    auto window_part = [&](cplx (&Y)[P], auto LIc, auto COc, auto E0c, auto E1c) __attribute__((always_inline)) {
      constexpr int li = decltype(LIc)::value, co = decltype(COc)::value;
#pragma unroll
      for (int e = decltype(E0c)::value; e < decltype(E1c)::value; ++e) {
        const int ro = e % K1, q = e / K1;
        const int t = (li * K1 + co) * K1 * L + e;
        const cplx gv = g[t % PF];
#pragma unroll
        for (int c = 0; c < P; ++c) {
          const cplx x = X[q][2 * c + ro];
          if (e == 0) {  // fma(a, b, 0) == a * b: same bits as accumulating from 0
            Y[c].re = __builtin_fma(x.re, gv.re, -x.im * gv.im);
            Y[c].im = __builtin_fma(x.re, gv.im, x.im * gv.re);
          } else {
            Y[c].re = __builtin_fma(x.re, gv.re, __builtin_fma(-x.im, gv.im, Y[c].re));
            Y[c].im = __builtin_fma(x.re, gv.im, __builtin_fma(x.im, gv.re, Y[c].im));
          }
        }
        // refill: the loads of a step are spread over its six product windows (§4.11)
        g[t % PF] = t + PF < NKEY ? key_load(key_step, t + PF) : key_load(key_next, t + PF - NKEY);
      }
    };
    // a finished window goes into the mailboxes of the waves (ct, co) at my position.  Before a
    // limb's first window is sent, every wave must have read the previous exchange (the last
    // forward level, or the previous limb's Y).
    auto window_send = [&](cplx (&Y)[P], auto COc) __attribute__((always_inline)) {
      constexpr int co = decltype(COc)::value;
#pragma unroll
      for (int c = 0; c < P; ++c) pin(Y[c]);
      if (co == 0) spin_until_ge(ctr, NW * rcnt, guard);
#pragma unroll
      for (int c = 0; c < P; ++c) mbox_all[(2 * c + co) * MB + w * 64 + lane] = Y[c];
    };
    constexpr std::integral_constant<int, 0> I0{};
    constexpr std::integral_constant<int, K1 * L> IE{};
    // the first four products of a level-major window need levels 0 and 1 only
    constexpr std::integral_constant<int, 2 * K1> IQ2{};
    auto window = [&](auto LIc, auto COc) __attribute__((always_inline)) {
      cplx Y[P];
      window_part(Y, LIc, COc, I0, IE);
      window_send(Y, COc);
    };
    auto digits = [&](cplx (&v)[8], int q) __attribute__((always_inline)) {
      if constexpr (BL != 0) {
        double d[16];
#pragma unroll
        for (int m = 0; m < 16; ++m) d[m] = decomp_word_digit<BL, L>(st[m], q);
#pragma unroll
        for (int m = 0; m < 8; ++m) v[m] = {d[m], d[m + 8]};
      } else {
        int32_t d[16];
#pragma unroll
        for (int m = 0; m < 16; ++m)
          d[m] = decomp_level32(st[m], (uint32_t)(q * logB), logB, half_m1, neg_base, q + 1 < L);
#pragma unroll
        for (int m = 0; m < 8; ++m) v[m] = {(double)d[m], (double)d[m + 8]};
      }
    };
    cplx Y0[P];  // window (limb 0, output 0), begun inside the third transform
    cplx hold[8];  // the level-0 spectrum during the second transform
#pragma unroll
    for (int q = 0; q < L; ++q) {
      cplx v[8];
      digits(v, q);
      cplx tw2[4];
      fwd_p2_tw(tw2, T, hi);
      // issued here, ahead of pass 1 and the register transpose that hide their latency
      __builtin_amdgcn_sched_barrier(0);
      // Levels 0 and 1 are traded in one exchange: level 0 waits in registers during the second
      // transform, then goes to my mailbox and level 1 to my transpose scratch (idle between
      // transforms).  The third transform overwrites that scratch, so it first waits (right
      // before its first LDS write) until every wave has read the pair.
      if (q == 2) {
        // the third transform with the first window's level-0/1 products behind its transpose's
        // writes and reads (the reads queue behind the writes: LDS operations of a wave execute
        // in issue order)
        fwd_p1(v);
        xpose_hi(v);
        geo8<false>(v, tw2);
        spin_until_ge(ctr, NW * rcnt, guard);
        fwd_w2(v, xch, hi, lo);
        wave_lds_fence();
        fwd_r2(v, xch, hi, lo);
        wave_lds_fence();
        slot_order();
        window_part(Y0, I0, I0, I0, IQ2);
        slot_order();
        geo8<false>(v, tw3);
      } else {
        fft512_fwd_tw(v, xch, lane, tw2, tw3, 0ull, []() __attribute__((always_inline)) {});
      }
      if (q == 0) {
#pragma unroll
        for (int k = 0; k < 8; ++k) hold[k] = v[k];
      } else {
#pragma unroll
        for (int k = 0; k < 8; ++k) {
          if (q == 1) mybox[k * 64] = hold[k], xch[k * 64 + lane] = v[k];
          else mybox[k * 64] = v[k];
        }
        lap(1);
        pair_barrier();
        lap(5);
#pragma unroll
        for (int u = 0; u < NW; ++u) {
          if (q == 1) X[0][u] = slotbox[u * MB], X[1][u] = xch_all[u * XS + w * 64 + lane];
          else X[2][u] = slotbox[u * MB];
        }
        slot_signal(ctr, lane, rcnt);
      }
    }
    lap(1);

    // ---- per limb: products of my slot for the 4 ciphertexts and both outputs (key from
    //      registers, refilled PF values ahead), Y exchange, inverse of my polynomial.
    // recombine: v is the inverse's pass-3 output without its last twiddle conj(psi^m),
    // psi^m = c (1 + i t): v conj(psi^m) = c (u + i u'), u = re + t im, u' = im - t re, and the
    // product c u is rounded once, into the integer (RND_MAGIC - c u as one FMA).
    auto recombine = [&](const cplx (&v)[8], auto LIc) __attribute__((always_inline)) {
      constexpr int lr = decltype(LIc)::value;
      // with a fixed base limb 2's rounding constant also removes limb 0's (fixed_limb_add)
      constexpr double RND = BL != 0 ? fixed_rnd_magic<lr>() : RND_MAGIC;
      // an FMA takes one scalar constant: the rounding constant goes through a vector register
      // pair, set here instead of held for the whole step loop
      double rnd = RND;
      pin(rnd);
#pragma unroll
      for (int m = 0; m < 8; ++m) {
        double tr, ti;
        if (m > 0) {
          // m > 4: psi^m = s (cot + i) with s = cos(pi (8 - m) / 16) and cot = tan(pi (8 - m) / 16),
          // the constants of 8 - m (no tangent above 1, 7 scalar constants in all: 13 spill SGPRs)
          const bool cot = m > 4;
          const double c = psi_pow(cot ? 8 - m : m).re, t = psi_tan(cot ? 8 - m : m);
          const double ur = cot ? __builtin_fma(t, v[m].re, v[m].im) : __builtin_fma(t, v[m].im, v[m].re);
          const double ui = cot ? __builtin_fma(t, v[m].im, -v[m].re) : __builtin_fma(-t, v[m].re, v[m].im);
          if constexpr (RESID) {  // the residual is taken on the value that is rounded
            double pr = c * ur, pi = c * ui;
            pin(pr), pin(pi);
            tr = RND - pr, ti = RND - pi;
            max_resid = fmax(max_resid, fabs(pr - (RND - tr)));
            max_resid = fmax(max_resid, fabs(pi - (RND - ti)));
          } else {
            tr = __builtin_fma(-c, ur, rnd), ti = __builtin_fma(-c, ui, rnd);
          }
        } else {
          tr = RND - v[m].re, ti = RND - v[m].im;
          if constexpr (RESID) {
            max_resid = fmax(max_resid, fabs(v[m].re - (RND - tr)));
            max_resid = fmax(max_resid, fabs(v[m].im - (RND - ti)));
          }
        }
        if constexpr (BL != 0) fixed_limb_add<lr>(B[m], B[m + 8], tr, ti);
        else limb_add<lr>(B[m], B[m + 8], tr, ti);
      }
    };
    // The first window of limb li + 1 runs between the reads of limb li's Y and its inverse, so the
    // reads' latency (and the other waves' reads, which that window's mailbox writes wait for) is
    // covered by 96 FMAs instead of being exposed right behind the barrier.
    window_part(Y0, I0, I0, IQ2, IE);  // the level-2 products cover the rest of the X[2] reads
    window_send(Y0, I0);
    static_for<0, LIMBS>([&](auto LI) __attribute__((always_inline)) {
      constexpr int li = decltype(LI)::value;
      constexpr std::integral_constant<int, 1> I1{};
      constexpr std::integral_constant<int, li + 1> LN{};
      window(LI, I1);
      lap(2);
      pair_barrier();
      lap(5);
      cplx vp[8];
#pragma unroll
      for (int k = 0; k < 8; ++k) vp[k] = mybox[k * 64];
      slot_signal(ctr, lane, rcnt);
      lap(3);
      cplx gi2[4];  // inverse pass-2 stage twiddles, read ahead of the transpose
      if constexpr (li + 1 < LIMBS) {
        window(LN, I0);
        lap(2);
      }
      inv_p2_stage_tw(gi2, T, lo);
      inv_p1(vp, 0ull);
      inv_w1(vp, xch, hi, lo);
      wave_lds_fence();
      inv_r1(vp, xch, hi, lo);
      wave_lds_fence();
      {  // the rest of the inverse (fft512_inv_tw): pass 2, its output twiddles (read after the
         // transpose: their latency hides behind the butterflies), hi transpose, pass 3
        cplx t1[8];
#pragma unroll
        for (int t = 0; t < 8; ++t) t1[t] = T.T1[hi * T1_STRIDE + 8 * t + lo];
        geo8<true, true>(vp, gi2);
#pragma unroll
        for (int t = 0; t < 8; ++t) vp[t] = cmulc(vp[t], t1[t]);
        xpose_hi(vp);
        dft8<true>(vp);  // pass 3 without its last twiddle: conj(psi^m) is applied by recombine
      }
      recombine(vp, LI);
      // materialise B here (else the inverse tail sinks into the next limb's products)
#pragma unroll
      for (int m = 0; m < 16; ++m) pin(B[m]);
      if constexpr (RESID) pin(max_resid);
      lap(4);
    });
  }

  if constexpr (STAMPS) {
    acc_t[6] = stamp() - t_begin;
    if (lane == 0 && resid_out) {
      unsigned long long* dst = resid_out + ((uint64_t)blockIdx.x * NW + w) * NSTAMP;
      for (int q = 0; q < NSTAMP; ++q) dst[q] = acc_t[q];
    }
  }

  // ---- sample extract (nth = 0) of acc = -B (pbs1024_pair_kernel).  In the RESID build the lane
  //      index, needed again only here, is the one value spilled across the step loop: it is taken
  //      again (mbcnt of a full mask).  The plain build has no spill and loses 0.8 % to the recompute.
  const int lane_x = RESID ? (int)__builtin_amdgcn_mbcnt_hi(~0u, __builtin_amdgcn_mbcnt_lo(~0u, 0u)) : lane;
  uint64_t* o = out + (active ? (out_idx ? out_idx[s] : s) : 0) * (uint64_t)(K * N + 1);
  if (!active) {
  } else if (h == 0) {
#pragma unroll
    for (int m = 0; m < 16; ++m) xch64[lane + 64 * m] = B[m];
    wave_lds_fence();
#pragma unroll
    for (int m = 0; m < 16; ++m) {
      const int j = lane_x + 64 * m;
      const uint64_t v = xch64[(N - j) & (N - 1)];
      o[j] = j == 0 ? 0ull - v : v;
    }
  } else if (lane_x == 0) {
    o[K * N] = 0ull - B[0];
  }

  if constexpr (RESID && !STAMPS) report_resid(max_resid, lane_x, active, resid_out);
}

// ------------------------------------------------------------------------------------
// host launchers
// ------------------------------------------------------------------------------------
// An integer override from the environment, `unset` when absent.  Read per call: tests and A/B
// runs switch CONCRETE_HIP_PBS_PAIRS / _QUAD / _HEX / _SLOT between calls.
static int env_int(const char* name, int unset) {
  const char* e = getenv(name);
  return e ? atoi(e) : unset;
}
// CONCRETE_HIP_PBS_STAMPS=1 (read once): the s_memtime-instrumented builds, with `resid` pointing at
// NSTAMP u64 per wave of the grid (per-wave cycle sums)
static bool env_set(const char* name) { return getenv(name) != nullptr; }
static bool stamps_build() {
  static const bool stamps = env_int("CONCRETE_HIP_PBS_STAMPS", 0) != 0;
  return stamps;
}

template <int BL, bool RESID, bool STAMPS>
static int launch_slot_t(const PbsArgs& a) {
  constexpr int P = PBS_PAIRS;
  const size_t lds = pbs1024_pair_slot_lds_bytes();
  static_assert(pbs1024_pair_slot_lds_bytes() <= 160 * 1024, "LDS of one CU");
  if (!pbs1024_exact(1, 3, a.base_log)) {
    set_error("pbs: N=1024 l=3 logB=%u is outside the exact range", a.base_log);
    return -2;
  }
  return launch_fused(pbs1024_pair_slot_kernel<BL, RESID, STAMPS>, P, P * 128, lds, a);
}

// the slot-split kernel (4 ciphertexts per workgroup, l = 3); with CONCRETE_HIP_PBS_STAMPS=1 its
// instrumented build (`resid`: 8 * ceil(num_samples / 4) * NSTAMP u64).  base_log 7 (cfg2) runs the
// instance with the base fixed at compile time; every other base of the exact range, and the
// instrumented build, the one that reads it at run time.
static int launch_slot(const PbsArgs& a) {
  if (stamps_build()) return launch_slot_t<0, true, true>(a);
  if (a.base_log == 7) return a.resid ? launch_slot_t<7, true, false>(a) : launch_slot_t<7, false, false>(a);
  return a.resid ? launch_slot_t<0, true, false>(a) : launch_slot_t<0, false, false>(a);
}

template <int P, int L, bool RESID, bool STAMPS>
static int launch_pair_t(const PbsArgs& a) {
  const size_t lds = pbs1024_pair_lds_bytes(L, P);
  // the exactness gate (pbs1024_exact) keeps l * logB <= 27: the decomposer state fits 32 bits
  if (!pbs1024_exact(1, L, a.base_log)) {
    set_error("pbs: N=1024 l=%d logB=%u is outside the exact range", L, a.base_log);
    return -2;
  }
  return launch_fused(pbs1024_pair_kernel<P, L, RESID, STAMPS>, P, P * 128, lds, a);
}

// compute units of the current device (cached per device)
static uint32_t device_cus() {
  static uint32_t cus[64] = {};
  int dev = 0;
  CHIP_CHECK(hipGetDevice(&dev));
  if (dev < 0 || dev >= 64) return 256;
  if (!cus[dev]) {
    int n = 0;
    CHIP_CHECK(hipDeviceGetAttribute(&n, hipDeviceAttributeMultiprocessorCount, dev));
    cus[dev] = n > 0 ? (uint32_t)n : 256u;
  }
  return cus[dev];
}

template <int P, int L>
static int launch_pair_p(const PbsArgs& a) {
  // stamps: `resid` holds 2 * P * ceil(num_samples / P) * NSTAMP u64
  if (stamps_build()) return launch_pair_t<P, L, true, true>(a);
  return a.resid ? launch_pair_t<P, L, true, false>(a) : launch_pair_t<P, L, false, false>(a);
}

// the contiguous part [start, start + count) of a batched call: the index arrays (the runtime's u64
// in / out / LUT indexes, wrappers.cpp:215-232) advance with it, or without them the LWE rows do
static PbsArgs pbs_args_range(const PbsArgs& a, uint32_t start, uint32_t count) {
  PbsArgs r = a;
  r.num_samples = count;
  if (a.in_idx) r.in_idx = a.in_idx + start;
  else r.in = a.in + (uint64_t)start * (a.n + 1);
  if (a.out_idx) r.out_idx = a.out_idx + start;
  else r.out = a.out + (uint64_t)start * (a.k * a.N + 1);
  if (a.lut_idx) r.lut_idx = a.lut_idx + start;
  return r;
}

template <int L>
static int launch_pair(const PbsArgs& a) {
  if (a.num_samples == 0) return 0;
  // Dispatch (the measurements behind each rule: DESIGN.md §4.1, §4.11, §4.13, §4.16).  Overrides, each
  // 0 = off, unset = automatic:
  //   CONCRETE_HIP_PBS_SLOT=1         the slot kernel for the whole call (l = 3)
  //   CONCRETE_HIP_PBS_HEX=1 / 2      the six-wave kernel, that many ciphertexts per workgroup (l = 3)
  //   CONCRETE_HIP_PBS_QUAD=1 / 2     the four-wave kernel (l = 3, batches the ring kernel would run at
  //                                   1 or 2 ciphertexts per workgroup)
  //   CONCRETE_HIP_PBS_PAIRS=1 / 2 / 4  the ring kernel with that many ciphertexts per workgroup
  // Automatic, l = 3, no PAIRS / QUAD override and no stamps: the call is split by pbs1024_plan.hpp into
  // whole rounds of 4 x CUs ciphertexts for the slot kernel (SLOT=0: the ring kernel, the A/B switch),
  // six-wave rounds of 2 x CUs and at most one round of one ciphertext per workgroup, each part a
  // contiguous range of the batch on the caller's stream.
  // Otherwise the ring kernel: a workgroup runs alone on its CU (LDS), so it takes 1 ciphertext per
  // workgroup at <= CUs ciphertexts, 2 at <= 2 x CUs, else 4; at l = 3 and 1 per workgroup the
  // four-wave kernel takes the call instead (QUAD=0 keeps the ring kernel).
  const int forced = env_int("CONCRETE_HIP_PBS_PAIRS", 0);
  const bool pairs_set = env_set("CONCRETE_HIP_PBS_PAIRS"), quad_set = env_set("CONCRETE_HIP_PBS_QUAD");
  const bool stamps_set = env_set("CONCRETE_HIP_PBS_STAMPS");  // set at all, even to 0: no plan, no four-wave kernel
  const uint32_t cus = device_cus();
  const int P = forced == 1 || forced == 2 || forced == 4 ? forced
                : a.num_samples <= cus ? 1 : a.num_samples <= 2 * cus ? 2 : 4;
  if (L == 3) {
    const int sl = env_int("CONCRETE_HIP_PBS_SLOT", -1);
    if (sl == 1) return launch_slot(a);
    const int hx = env_int("CONCRETE_HIP_PBS_HEX", -1);
    if (hx == 1 || hx == 2) return pbs1024_hex_launch(a, hx);
    if (hx != 0 && !pairs_set && !quad_set && !stamps_set) {
      const Pbs1024Plan plan = plan_pbs1024(a.num_samples, cus);
      uint32_t start = 0;
      int rc = 0;
      if (plan.pair) {
        const PbsArgs part = pbs_args_range(a, start, plan.pair);
        rc = sl == 0 ? launch_pair_p<4, L>(part) : launch_slot(part);
        start += plan.pair;
      }
      if (rc == 0 && plan.hex2) {
        rc = pbs1024_hex_launch(pbs_args_range(a, start, plan.hex2), 2);
        start += plan.hex2;
      }
      if (rc == 0 && plan.hex1) rc = pbs1024_hex_launch(pbs_args_range(a, start, plan.hex1), 1);
      return rc;
    }
  }
  if (L == 3 && P <= 2 && !stamps_set) {
    const int q = env_int("CONCRETE_HIP_PBS_QUAD", -1);
    if (q == 1 || q == 2) return pbs1024_quad_launch(a, q);
    if (q != 0 && P == 1) return pbs1024_quad_launch(a, 1);
  }
  if (P == 1) return launch_pair_p<1, L>(a);
  if (P == 2) return launch_pair_p<2, L>(a);
  return launch_pair_p<4, L>(a);
}

int pbs_launch(const PbsArgs& a) {
  const KeyKind kind = key_format(a.k, a.N, a.level).kind;
  if (kind == KeyKind::GENERIC) return pbs_generic_launch(a);
  if (kind == KeyKind::N2048) return pbs2048_launch(a);
  if (kind == KeyKind::K2N1024) return pbs1024k2_launch(a);
  if (kind == KeyKind::SMALL) return pbs_small_launch(a);
  if (kind == KeyKind::N1024 && a.limbs == 3) {
    switch (a.level) {
      case 1: return launch_pair<1>(a);
      case 2: return launch_pair<2>(a);
      case 3: return launch_pair<3>(a);
      default: break;
    }
  }
  set_error("unsupported PBS parameters: N=%u k=%u level=%u limbs=%u", a.N, a.k, a.level, a.limbs);
  return -2;
}

}  // namespace chip
