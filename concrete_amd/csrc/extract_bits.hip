// extract_bits.hip — batched LWE bit extraction, stage 1 of the WoP-PBS (concrete-cpu
// src/c_api/wop_pbs.rs:118-212, concrete-cuda cuda_extract_bits_64).
//
// Per input ciphertext c of dimension kN, with nb = number_of_bits and dl = delta_log (wrapping u64):
//   c' = c
//   for t = 0 .. nb-1:
//     u = KS(c' << (64 - dl - t - 1));  out[nb-1-t] = u;  stop after the last bit
//     u.body += 2^62;  v = PBS(u, acc(dl-1+t));  v.body += 2^(dl-1+t);  c' -= v
// acc(e): the trivial GLWE whose body polynomial has every coefficient -(2^e).
//
// The keyswitch and the PBS are the library's exact kernels (keyswitch_launch, pbs_launch /
// pbs_generic_launch).  What sits between them is one HBM-bound stream per iteration, eb_step_kernel:
// it folds the previous PBS output and its body constant into the running copy c', stores it, and
// writes the shifted copy the keyswitch reads.  Rows carry their own (nb, dl); the host orders them
// by decreasing nb, so the rows that still keyswitch (nb > t) and those that still bootstrap
// (nb > t + 1) are prefixes and both kernels run on shrinking sample counts through index arrays
// uploaded once per call.  Nothing between the iterations touches the host.
#include "../../include/concrete_hip.h"

#include <algorithm>
#include <numeric>
#include <vector>

#include "common.hpp"
#include "pbs.hpp"
#include "companion.hpp"

namespace chip {

constexpr uint32_t EB_MAX_BITS = 63;  // dl >= 1 and dl + nb <= 64
constexpr uint32_t EB_MAX_ACCS = 63;  // accumulators differ by e = dl - 1 + t only, e in 0 .. 62

// One word of the step.  FIRST (t = 0): the running copy starts as the caller's input row; later
// iterations subtract the previous PBS output v and, on the body, its constant 2^(dl-2+t).
template <bool FIRST>
__device__ __forceinline__ uint64_t eb_fold(uint64_t c, uint64_t v, bool body, uint32_t dl, uint32_t t) {
  if constexpr (FIRST) return c;
  uint64_t x = c - v;
  if (body) x -= 1ull << (dl - 2 + t);
  return x;
}

// Rows 0 .. rows-1 of the sorted order, `total` = rows * W words.  One thread per 2 words: the running
// copy, the PBS output and the keyswitch input share one row-major layout with 16-B aligned bases, so
// every pair is one 16-B access (the t = 0 gather from the caller's rows, of odd width, is per word).
template <bool FIRST>
__global__ void __launch_bounds__(256) eb_step_kernel(uint64_t* __restrict__ copy, uint64_t* __restrict__ ks_in,
                                                      const uint64_t* __restrict__ src,
                                                      const uint64_t* __restrict__ in_row,
                                                      const uint32_t* __restrict__ dl, uint32_t t, uint64_t W,
                                                      uint64_t total) {
  const uint64_t stride = (uint64_t)gridDim.x * blockDim.x * 2;
  for (uint64_t e = ((uint64_t)blockIdx.x * blockDim.x + threadIdx.x) * 2; e < total; e += stride) {
    const uint64_t r0 = e / W, c0 = e - r0 * W;
    const uint32_t d0 = dl[r0];
    if (e + 1 < total) {
      const bool wrap = c0 + 1 == W;
      const uint64_t r1 = wrap ? r0 + 1 : r0, c1 = wrap ? 0 : c0 + 1;
      const uint32_t d1 = wrap ? dl[r1] : d0;
      ulonglong2 x;
      if constexpr (FIRST) {
        x.x = src[in_row[r0] * W + c0];
        x.y = src[in_row[r1] * W + c1];
      } else {
        const ulonglong2 c = *reinterpret_cast<const ulonglong2*>(copy + e);
        const ulonglong2 v = *reinterpret_cast<const ulonglong2*>(src + e);
        x.x = eb_fold<false>(c.x, v.x, c0 == W - 1, d0, t);
        x.y = eb_fold<false>(c.y, v.y, c1 == W - 1, d1, t);
      }
      *reinterpret_cast<ulonglong2*>(copy + e) = x;
      ulonglong2 s;
      s.x = x.x << (63 - d0 - t);
      s.y = x.y << (63 - d1 - t);
      *reinterpret_cast<ulonglong2*>(ks_in + e) = s;
    } else {
      const uint64_t x = FIRST ? src[in_row[r0] * W + c0] : eb_fold<false>(copy[e], src[e], c0 == W - 1, d0, t);
      copy[e] = x;
      ks_in[e] = x << (63 - d0 - t);
    }
  }
}

// The call's accumulator table: slot i = k zero polynomials, then N coefficients -(2^exps[i]).
// G = (k+1) N and the mask length kN are even, so a pair never straddles a boundary.
__global__ void __launch_bounds__(256) eb_acc_kernel(uint64_t* __restrict__ acc, const uint32_t* __restrict__ exps,
                                                     uint64_t G, uint64_t mask_len, uint64_t total) {
  const uint64_t stride = (uint64_t)gridDim.x * blockDim.x * 2;
  for (uint64_t e = ((uint64_t)blockIdx.x * blockDim.x + threadIdx.x) * 2; e < total; e += stride) {
    const uint64_t slot = e / G, j = e - slot * G;
    const uint64_t v = j < mask_len ? 0ull : 0ull - (1ull << exps[slot]);
    ulonglong2 x;
    x.x = v, x.y = v;
    *reinterpret_cast<ulonglong2*>(acc + e) = x;
  }
}

// The PBS input of the rows that go on: the keyswitch output just written to the caller's rows
// (which must stay as the keyswitch left them), body + 2^62.  rows x (n+1) words, a small stream.
__global__ void __launch_bounds__(256) eb_pbs_in_kernel(uint64_t* __restrict__ pbs_in, const uint64_t* __restrict__ out,
                                                        const uint64_t* __restrict__ out_idx, uint64_t w,
                                                        uint64_t total) {
  const uint64_t stride = (uint64_t)gridDim.x * blockDim.x;
  for (uint64_t e = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; e < total; e += stride) {
    const uint64_t r = e / w, c = e - r * w;
    uint64_t v = out[out_idx[r] * w + c];
    if (c == w - 1) v += 1ull << 62;
    pbs_in[e] = v;
  }
}

static uint32_t eb_blocks(uint64_t threads) {
  return (uint32_t)std::min<uint64_t>((threads + 255) / 256, 256ull * 64);
}

static uint64_t align16(uint64_t bytes) { return (bytes + 15) & ~15ull; }

// Scratch segments, each 16-B aligned: running copy, keyswitch input, PBS output (B x (kN+1) each),
// PBS input (B x (n+1)), the accumulator table, then the index data in the order it is uploaded.
struct EbLayout {
  uint64_t copy, ks_in, pbs_out, pbs_in, acc, idx, bytes;
};
static uint32_t eb_acc_slots(uint64_t B, uint32_t max_bits) {
  return (uint32_t)std::max<uint64_t>(1, std::min<uint64_t>(EB_MAX_ACCS, B * (uint64_t)(max_bits - 1)));
}
// bytes of index data for B rows whose bit counts sum to `bits` (keyswitch rows) and to `bits - B`
// PBS rows: in_row (u64), keyswitch output rows (u64), LUT indexes (u64), dl (u32), exponents (u32)
static uint64_t eb_idx_bytes(uint64_t B, uint64_t bits, uint32_t slots) {
  return align16(8 * B + 8 * bits + 8 * (bits - B) + 4 * B + 4 * (uint64_t)slots);
}
static EbLayout eb_layout(uint64_t B, uint64_t W, uint64_t w, uint64_t G, uint32_t max_bits) {
  EbLayout l;
  const uint64_t big = align16(8 * B * W);
  l.copy = 0;
  l.ks_in = big;
  l.pbs_out = 2 * big;
  l.pbs_in = 3 * big;
  l.acc = l.pbs_in + align16(8 * B * w);
  const uint32_t slots = eb_acc_slots(B, max_bits);
  l.idx = l.acc + align16(8 * G * slots);
  l.bytes = l.idx + eb_idx_bytes(B, B * max_bits, slots);
  return l;
}

// Page-locked staging of the index data, one grow-only block per host thread.  The upload is
// asynchronous; the event lets the thread's next call wait for exactly that copy (normally long
// done) before it overwrites the block, so no call synchronises its stream.
struct EbStaging {
  void* p = nullptr;
  uint64_t cap = 0;
  hipEvent_t ev = nullptr;
  int dev = -1;
};
static void* eb_stage(EbStaging& st, uint64_t bytes, int dev) {
  if (st.ev) CHIP_CHECK(hipEventSynchronize(st.ev));
  if (st.ev && st.dev != dev) {
    CHIP_CHECK(hipEventDestroy(st.ev));
    st.ev = nullptr;
  }
  if (!st.ev) {
    CHIP_CHECK(hipEventCreateWithFlags(&st.ev, hipEventDisableTiming));
    st.dev = dev;
  }
  if (st.cap < bytes) {
    if (st.p) CHIP_CHECK(hipHostFree(st.p));
    st.p = nullptr, st.cap = 0;
    CHIP_CHECK(hipHostMalloc(&st.p, bytes, hipHostMallocPortable));
    st.cap = bytes;
  }
  return st.p;
}

static bool eb_params_ok(uint32_t n_in, uint32_t n_out, uint32_t k, uint32_t N, uint32_t base_log_bsk,
                         uint32_t level_bsk, uint32_t base_log_ksk, uint32_t level_ksk) {
  const bool pbs = pbs_params_ok(k, N, level_bsk, base_log_bsk) || pbs_needs_generic_key(k, N, level_bsk, base_log_bsk);
  return pbs && keyswitch_params_ok(level_ksk, base_log_ksk, n_in, n_out);
}

}  // namespace chip

using namespace chip;

extern "C" {

int concrete_hip_extract_bits_supported(uint32_t lwe_dimension_in, uint32_t lwe_dimension_out,
                                        uint32_t glwe_dimension, uint32_t polynomial_size, uint32_t base_log_bsk,
                                        uint32_t level_count_bsk, uint32_t base_log_ksk, uint32_t level_count_ksk) {
  if ((uint64_t)glwe_dimension * polynomial_size != lwe_dimension_in || lwe_dimension_out == 0) return 0;
  return eb_params_ok(lwe_dimension_in, lwe_dimension_out, glwe_dimension, polynomial_size, base_log_bsk,
                      level_count_bsk, base_log_ksk, level_count_ksk)
             ? 1
             : 0;
}

uint64_t concrete_hip_extract_bits_scratch_bytes(uint32_t lwe_dimension_in, uint32_t lwe_dimension_out,
                                                 uint32_t glwe_dimension, uint32_t polynomial_size,
                                                 uint32_t num_samples, uint32_t max_number_of_bits) {
  if (num_samples == 0 || max_number_of_bits == 0 || max_number_of_bits > EB_MAX_BITS) return 0;
  return eb_layout(num_samples, (uint64_t)lwe_dimension_in + 1, (uint64_t)lwe_dimension_out + 1,
                   ((uint64_t)glwe_dimension + 1) * polynomial_size, max_number_of_bits)
      .bytes;
}

int concrete_hip_extract_bits(void* stream, uint32_t gpu_index, uint64_t* lwe_array_out, const uint64_t* lwe_array_in,
                              const void* fourier_bsk, const uint64_t* ksk, const uint32_t* number_of_bits,
                              const uint32_t* delta_log, const uint64_t* out_row_offsets, uint32_t lwe_dimension_in,
                              uint32_t lwe_dimension_out, uint32_t glwe_dimension, uint32_t polynomial_size,
                              uint32_t base_log_bsk, uint32_t level_count_bsk, uint32_t base_log_ksk,
                              uint32_t level_count_ksk, uint32_t num_samples, void* scratch, uint64_t scratch_bytes) {
  // ---- validation: nothing below this block runs, and no HIP call is made, on a refused call ----
  if (num_samples == 0) return 0;
  if (!lwe_array_out || !lwe_array_in || !fourier_bsk || !ksk || !number_of_bits || !delta_log) {
    set_error("extract_bits: null pointer");
    return -1;
  }
  const uint64_t B = num_samples;
  uint64_t bits = 0;
  uint32_t max_bits = 0;
  for (uint64_t i = 0; i < B; ++i) {
    const uint32_t nb = number_of_bits[i], dl = delta_log[i];
    if (nb == 0 || dl == 0 || (uint64_t)dl + nb > 64) {
      set_error("extract_bits: row %llu has number_of_bits=%u delta_log=%u (need nb >= 1, dl >= 1, dl + nb <= 64)",
                (unsigned long long)i, nb, dl);
      return -3;
    }
    bits += nb;
    max_bits = std::max(max_bits, nb);
  }
  if ((uint64_t)glwe_dimension * polynomial_size != lwe_dimension_in || lwe_dimension_out == 0) {
    set_error("extract_bits: lwe_dimension_in=%u must be glwe_dimension * polynomial_size = %u * %u, and "
              "lwe_dimension_out=%u > 0",
              lwe_dimension_in, glwe_dimension, polynomial_size, lwe_dimension_out);
    return -3;
  }
  if (out_row_offsets) {
    // the output is the packed array of sum(nb) rows: the blocks may be placed in any order, but
    // inside it and apart from each other
    std::vector<uint64_t> by_off(B);
    std::iota(by_off.begin(), by_off.end(), 0ull);
    std::sort(by_off.begin(), by_off.end(),
              [&](uint64_t a, uint64_t b) { return out_row_offsets[a] < out_row_offsets[b]; });
    uint64_t end = 0;
    for (uint64_t i : by_off) {
      const uint64_t off = out_row_offsets[i];
      if (off >= bits || bits - off < number_of_bits[i]) {
        set_error("extract_bits: output block of row %llu (rows %llu .. +%u) is outside the %llu output rows",
                  (unsigned long long)i, (unsigned long long)off, number_of_bits[i], (unsigned long long)bits);
        return -3;
      }
      if (off < end) {
        set_error("extract_bits: output block of row %llu (from row %llu) overlaps another block",
                  (unsigned long long)i, (unsigned long long)off);
        return -3;
      }
      end = off + number_of_bits[i];
    }
  }
  if (!eb_params_ok(lwe_dimension_in, lwe_dimension_out, glwe_dimension, polynomial_size, base_log_bsk,
                    level_count_bsk, base_log_ksk, level_count_ksk)) {
    set_error("extract_bits: unsupported parameters k=%u N=%u bsk level=%u base_log=%u, ksk %u -> %u level=%u "
              "base_log=%u",
              glwe_dimension, polynomial_size, level_count_bsk, base_log_bsk, lwe_dimension_in, lwe_dimension_out,
              level_count_ksk, base_log_ksk);
    return -2;
  }
  const uint64_t W = (uint64_t)lwe_dimension_in + 1, w = (uint64_t)lwe_dimension_out + 1;
  const uint64_t G = ((uint64_t)glwe_dimension + 1) * polynomial_size;
  const EbLayout lay = eb_layout(B, W, w, G, max_bits);
  if (const int rc = scratch_refused("extract_bits", scratch, scratch_bytes, lay.bytes)) return rc;

  // ---- schedule: rows by decreasing nb; active[t] = rows with nb > t (a prefix of that order) ----
  std::vector<uint32_t> order(B);
  std::iota(order.begin(), order.end(), 0u);
  std::stable_sort(order.begin(), order.end(),
                   [&](uint32_t a, uint32_t b) { return number_of_bits[a] > number_of_bits[b]; });
  std::vector<uint64_t> active(max_bits + 1, 0);
  for (uint64_t i = 0; i < B; ++i)
    for (uint32_t t = 0; t < number_of_bits[i]; ++t) ++active[t];
  // accumulator slots of the exponents e = dl - 1 + t the call uses
  int slot_of[EB_MAX_ACCS];
  std::fill(slot_of, slot_of + EB_MAX_ACCS, -1);
  for (uint64_t i = 0; i < B; ++i)
    for (uint32_t t = 0; t + 1 < number_of_bits[i]; ++t) slot_of[delta_log[i] - 1 + t] = 0;
  std::vector<uint32_t> exps;
  for (uint32_t e = 0; e < EB_MAX_ACCS; ++e)
    if (slot_of[e] == 0) slot_of[e] = (int)exps.size(), exps.push_back(e);
  const uint32_t slots = (uint32_t)exps.size();

  // ---- the key: concrete_hip_pbs's gates, refusing before anything is written ----
  PbsKey pk;
  if (const int rc = pbs_resolve_key(stream, gpu_index, fourier_bsk, lwe_dimension_out, glwe_dimension,
                                     polynomial_size, base_log_bsk, level_count_bsk, &pk))
    return rc;
  hipStream_t s = (hipStream_t)stream;

  // ---- index data, in upload order ----
  const uint64_t idx_bytes = eb_idx_bytes(B, bits, std::max(slots, 1u));
  static thread_local EbStaging staging;
  char* h = (char*)eb_stage(staging, idx_bytes, (int)gpu_index);
  uint64_t* h_in_row = (uint64_t*)h;
  uint64_t* h_ks_out = h_in_row + B;
  uint64_t* h_lut = h_ks_out + bits;
  uint32_t* h_dl = (uint32_t*)(h_lut + (bits - B));
  uint32_t* h_exps = h_dl + B;
  std::vector<uint64_t> first_row(B);  // packed placement: blocks in input order
  if (!out_row_offsets) {
    uint64_t at = 0;
    for (uint64_t i = 0; i < B; ++i) first_row[i] = at, at += number_of_bits[i];
  }
  for (uint64_t r = 0; r < B; ++r) h_in_row[r] = order[r], h_dl[r] = delta_log[order[r]];
  {
    uint64_t ko = 0, lo = 0;
    for (uint32_t t = 0; t < max_bits; ++t) {
      for (uint64_t r = 0; r < active[t]; ++r) {
        const uint32_t i = order[r];
        h_ks_out[ko + r] = (out_row_offsets ? out_row_offsets[i] : first_row[i]) + (number_of_bits[i] - 1 - t);
      }
      for (uint64_t r = 0; r < active[t + 1]; ++r) h_lut[lo + r] = (uint64_t)slot_of[delta_log[order[r]] - 1 + t];
      ko += active[t], lo += active[t + 1];
    }
  }
  for (uint32_t i = 0; i < slots; ++i) h_exps[i] = exps[i];

  const CallScratch own(scratch, lay.bytes, s);
  char* base = own.base;
  uint64_t* d_copy = (uint64_t*)(base + lay.copy);
  uint64_t* d_ks_in = (uint64_t*)(base + lay.ks_in);
  uint64_t* d_pbs_out = (uint64_t*)(base + lay.pbs_out);
  uint64_t* d_pbs_in = (uint64_t*)(base + lay.pbs_in);
  uint64_t* d_acc = (uint64_t*)(base + lay.acc);
  const uint64_t* d_in_row = (const uint64_t*)(base + lay.idx);
  const uint64_t* d_ks_out = d_in_row + B;
  const uint64_t* d_lut = d_ks_out + bits;
  const uint32_t* d_dl = (const uint32_t*)(d_lut + (bits - B));
  const uint32_t* d_exps = d_dl + B;
  CHIP_CHECK(hipMemcpyAsync(base + lay.idx, h, idx_bytes, hipMemcpyHostToDevice, s));
  CHIP_CHECK(hipEventRecord(staging.ev, s));
  if (slots) {
    const uint64_t total = G * slots;
    hipLaunchKernelGGL(eb_acc_kernel, dim3(eb_blocks(total / 2)), dim3(256), 0, s, d_acc, d_exps, G,
                       (uint64_t)lwe_dimension_in, total);
  }

  // ---- the loop: step, keyswitch into the caller's rows, PBS input, PBS; no host synchronisation ----
  int rc = 0;
  const SyncGuard guard = slots ? sync_guard((int)gpu_index, s) : SyncGuard{nullptr, 0};
  uint64_t ko = 0, lo = 0;
  for (uint32_t t = 0; t < max_bits && rc == 0; ++t) {
    const uint64_t A = active[t], P = active[t + 1], total = A * W;
    if (t == 0)
      hipLaunchKernelGGL((eb_step_kernel<true>), dim3(eb_blocks((total + 1) / 2)), dim3(256), 0, s, d_copy, d_ks_in,
                         lwe_array_in, d_in_row, d_dl, t, W, total);
    else
      hipLaunchKernelGGL((eb_step_kernel<false>), dim3(eb_blocks((total + 1) / 2)), dim3(256), 0, s, d_copy, d_ks_in,
                         (const uint64_t*)d_pbs_out, d_in_row, d_dl, t, W, total);
    KsArgs ka{s, lwe_array_out, d_ks_out + ko, d_ks_in, nullptr, ksk, lwe_dimension_in, lwe_dimension_out,
              base_log_ksk, level_count_ksk, (uint32_t)A};
    rc = keyswitch_launch(ka);
    if (rc != 0 || P == 0) break;
    hipLaunchKernelGGL(eb_pbs_in_kernel, dim3(eb_blocks(P * w)), dim3(256), 0, s, d_pbs_in,
                       (const uint64_t*)lwe_array_out, d_ks_out + ko, w, P * w);
    PbsArgs pa{s, d_pbs_out, nullptr, d_acc, d_lut + lo, d_pbs_in, nullptr, pk.key, lwe_dimension_out,
               glwe_dimension, polynomial_size, base_log_bsk, level_count_bsk, pk.limbs, (uint32_t)P, nullptr, guard};
    rc = pk.generic ? pbs_generic_launch(pa) : pbs_launch(pa);
    ko += A, lo += P;
  }
  const hipError_t e = hipGetLastError();
  if (rc == 0 && e != hipSuccess) {
    set_error("extract_bits launch failed: %s", hipGetErrorString(e));
    rc = -1;
  }
  return rc;
}

}  // extern "C"
