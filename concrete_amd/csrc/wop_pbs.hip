// wop_pbs.hip — the WoP-PBS end to end: the drivers that chain bit extraction (stage 1, extract_bits.hip),
// the circuit bootstrap (stage 2, circuit_bootstrap.hip) and vertical packing (stage 3, vertical_packing.hip),
// and the two small streams for the data the stages do not hand to each other (concrete-cuda
// cuda_circuit_bootstrap_vertical_packing_64 and cuda_wop_pbs_64, rust_api/src/cuda_bind.rs:650-813; the CPU
// runtime's memref_wop_pbs_crt_buffer, compiler lib/Runtime/wrappers.cpp:855-997).  All arithmetic mod 2^64.
//
// One lookup with t boolean inputs and tau LUTs of 2^t words, r = max(t - log2 N, 0), m = min(t, log2 N):
//   stage 2  over the t bit ciphertexts at delta_log 63: [t][level_cbs][k+1][(k+1)N], most significant bit first,
//            level matrix 0 = decomposition level 1: exactly stage 3's ggsw_in
//   stage 3  with (level, base_log) = (level_cbs, base_log_cbs), r, mbr_size = m, on the LUTs as [tau][2^r][N]:
//            the caller's array as it stands when t >= log2 N, else its 2^t words at the front of a zero
//            polynomial (concrete-cpu's Ordering::Less branch)
// CRT front (wrappers.cpp:903-965): block i of modulus m_i yields nb_i = ceil(log2 m_i) bits at delta_log
// 64 - nb_i after 2^(63-nb_i) - 2^(59-nb_i) is taken off its body (the second term dropped when nb_i > 59);
// per value the extracted rows are [bits of block n-1 | ... | bits of block 0], each most significant first.
//
// The stages are called through their public entry points, so their kernels, gates and refusals are theirs;
// the driver validates everything they would refuse for before its first device call, carves every
// intermediate buffer from one scratch buffer (the caller's, or one pool allocation), and adds no host
// synchronisation to the one stage 3 makes for its gate.  The stages run one after the other on one stream,
// so they share one scratch segment sized for the largest of them.
#include "../../include/concrete_hip.h"

#include <algorithm>
#include <vector>

#include "common.hpp"
#include "companion.hpp"

namespace chip {

constexpr uint32_t WOP_MAX_BLOCKS = 16;  // CRT blocks (stage-1 inputs) per value: their offsets travel by value
constexpr uint32_t WOP_MAX_R = 24;       // the CMUX tree's depth (vertical_packing.hip)

struct WopOffsets {
  uint64_t v[WOP_MAX_BLOCKS];
};

// The private copy of the CRT front: rows x W words, row r belonging to block r mod blocks; the block's
// offset comes off the body.  One word per thread, consecutive threads on consecutive words.
__global__ void __launch_bounds__(256) wop_front_kernel(uint64_t* __restrict__ out, const uint64_t* __restrict__ in,
                                                        const WopOffsets off, uint32_t blocks, uint64_t W,
                                                        uint64_t total) {
  const uint64_t stride = (uint64_t)gridDim.x * blockDim.x;
  for (uint64_t e = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; e < total; e += stride) {
    const uint64_t r = e / W, c = e - r * W;
    uint64_t v = in[e];
    if (c == W - 1) v -= off.v[r % blocks];
    out[e] = v;
  }
}

// LUT layout for t < log2 N: [tau][words] -> [tau][1][N], the words at the front, the rest zero.
__global__ void __launch_bounds__(256) wop_lut_pad_kernel(uint64_t* __restrict__ out, const uint64_t* __restrict__ in,
                                                          uint64_t words, uint64_t N, uint64_t total) {
  const uint64_t stride = (uint64_t)gridDim.x * blockDim.x;
  for (uint64_t e = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; e < total; e += stride) {
    const uint64_t o = e / N, j = e - o * N;
    out[e] = j < words ? in[o * words + j] : 0ull;
  }
}

static uint32_t wop_blocks(uint64_t threads) {
  return (uint32_t)std::min<uint64_t>((threads + 255) / 256, 256ull * 64);
}
static uint64_t align16(uint64_t bytes) { return (bytes + 15) & ~15ull; }
static uint32_t log2u(uint32_t N) { return 31u - (uint32_t)__builtin_clz(N); }
static uint32_t crt_bits(uint64_t modulus) {  // ceil(log2 m), m >= 2
  return 64u - (uint32_t)__builtin_clzll(modulus - 1);
}

// Scratch segments, each 16-byte aligned: the front's copy (batch x num_inputs x (kN+1)), the bit ciphertexts
// (batch x t x (n+1)) — both empty without stage 1 —, the GGSWs (batch x t x level_cbs x (k+1) x (k+1)N), the
// laid-out LUTs (tau x N, reserved whatever t is so that the size does not fall where t reaches log2 N), then
// the stages' shared scratch.  Stage 1's share is sized for rows of up to t - (num_inputs - 1) bits (every
// input has at least one), which the call's real largest bit count never exceeds.
struct WopLayout {
  uint64_t front, bits, ggsw, lut, stage, stage_bytes, bytes;
  uint32_t r, m;
  bool ok;
};
static WopLayout wop_layout(uint32_t n, uint32_t k, uint32_t N, uint32_t level_cbs, uint32_t num_inputs, uint32_t t,
                            uint32_t tau, uint32_t batch) {
  WopLayout l{};
  if (N == 0 || (N & (N - 1)) || t == 0 || tau == 0 || batch == 0 || level_cbs == 0 || n == 0 || k == 0) return l;
  if (num_inputs > t) return l;
  const uint32_t logN = log2u(N);
  l.r = t > logN ? t - logN : 0, l.m = std::min(t, logN);
  if (l.r > WOP_MAX_R) return l;
  typedef unsigned __int128 u128;
  const u128 W = (u128)k * N + 1, w = (u128)n + 1, G = ((u128)k + 1) * N;
  const u128 rows = (u128)batch * t, ins = (u128)batch * num_inputs;
  if (rows >> 32 || ins >> 32 || W >> 32 || G >> 32) return l;
  const u128 front = ins * W * 8, bits = num_inputs ? rows * w * 8 : 0;
  const u128 ggsw = rows * level_cbs * (k + 1) * G * 8, lut = (u128)tau * N * 8;
  if ((front + bits + ggsw + lut) >> 62) return l;
  uint64_t stage = 0;
  if (num_inputs) {
    const uint32_t max_bits = std::min<uint32_t>(63, t - (num_inputs - 1));
    const uint64_t eb = concrete_hip_extract_bits_scratch_bytes((uint32_t)(W - 1), n, k, N, (uint32_t)ins, max_bits);
    if (eb == 0) return l;
    stage = eb;
  }
  const uint64_t cbs = concrete_hip_circuit_bootstrap_scratch_bytes(n, k, N, level_cbs, (uint32_t)rows);
  const uint64_t vp = concrete_hip_vertical_packing_scratch_bytes(k, N, level_cbs, l.r, l.m, tau, batch);
  if (cbs == 0 || vp == 0) return l;
  stage = std::max(stage, std::max(cbs, vp));
  l.front = 0;
  l.bits = align16((uint64_t)front);
  l.ggsw = l.bits + align16((uint64_t)bits);
  l.lut = l.ggsw + align16((uint64_t)ggsw);
  l.stage = l.lut + align16((uint64_t)lut);
  l.stage_bytes = align16(stage);
  l.bytes = l.stage + l.stage_bytes;
  l.ok = !(l.bytes >> 62);
  return l;
}

// 0, or -1 with the message set when the launch just made failed
static int launch_refused(const char* who, const char* kernel) {
  const hipError_t e = hipGetLastError();
  if (e == hipSuccess) return 0;
  set_error("%s: %s launch failed: %s", who, kernel, hipGetErrorString(e));
  return -1;
}

static bool wop_params_ok(bool stage1, uint32_t n, uint32_t k, uint32_t N, uint32_t level_bsk, uint32_t base_log_bsk,
                          uint32_t level_ksk, uint32_t base_log_ksk, uint32_t level_pksk, uint32_t base_log_pksk,
                          uint32_t level_cbs, uint32_t base_log_cbs) {
  const uint64_t big = (uint64_t)k * N;
  if (stage1 && (big > 0xffffffffull || !concrete_hip_extract_bits_supported((uint32_t)big, n, k, N, base_log_bsk,
                                                                              level_bsk, base_log_ksk, level_ksk)))
    return false;
  return concrete_hip_circuit_bootstrap_supported(k, N, level_bsk, base_log_bsk, level_pksk, base_log_pksk, level_cbs,
                                                  base_log_cbs) &&
         concrete_hip_vertical_packing_supported(k, N, level_cbs, base_log_cbs);
}

// One chained call.  num_inputs > 0: lwe_in is [batch][num_inputs][kN+1] and stage 1 extracts nb[i] bits at
// dl[i] from input i of every value (offsets: the body offsets of the CRT front, or nullptr to read lwe_in as
// it stands; msb_last: input num_inputs-1 supplies the most significant bits, the CRT order).  num_inputs == 0:
// lwe_in is [batch][t][n+1], the bit ciphertexts at cbs_delta_log.
struct WopCall {
  const char* who = nullptr;
  void* stream = nullptr;
  uint32_t gpu = 0;
  uint64_t* lwe_out = nullptr;
  const uint64_t* lwe_in = nullptr;
  const uint64_t* luts = nullptr;
  const void* fbsk = nullptr;
  const uint64_t* ksk = nullptr;  // stage 1 only
  const uint64_t* fpksk = nullptr;
  uint32_t n = 0, k = 0, N = 0, level_bsk = 0, base_log_bsk = 0, level_ksk = 0, base_log_ksk = 0, level_pksk = 0,
           base_log_pksk = 0, level_cbs = 0, base_log_cbs = 0, cbs_delta_log = 63;
  uint32_t num_inputs = 0;  // 0: no stage 1
  const uint32_t* nb = nullptr;
  const uint32_t* dl = nullptr;
  const uint64_t* offsets = nullptr;
  bool msb_last = false;
  uint32_t t = 0, tau = 0, batch = 0;
  bool lut_padded = false;  // luts is [tau][max(2^t, N)] already
  void* scratch = nullptr;
  uint64_t scratch_bytes = 0;
  double* spectrum = nullptr;
};

// The fields of a call without stage 1, each by name; a caller with stage 1 adds ksk, its decomposition and the
// per-input arrays the same way.
struct WopShape {
  uint32_t n, k, N, level_bsk, base_log_bsk, level_pksk, base_log_pksk, level_cbs, base_log_cbs;
};
static WopCall wop_call(const char* who, void* stream, uint32_t gpu, void* lwe_out, const void* lwe_in,
                        const void* luts, const void* fbsk, const void* fpksk, const WopShape& sh, uint32_t t,
                        uint32_t tau, uint32_t batch, void* scratch, uint64_t scratch_bytes) {
  WopCall c;
  c.who = who, c.stream = stream, c.gpu = gpu;
  c.lwe_out = (uint64_t*)lwe_out, c.lwe_in = (const uint64_t*)lwe_in, c.luts = (const uint64_t*)luts;
  c.fbsk = fbsk, c.fpksk = (const uint64_t*)fpksk;
  c.n = sh.n, c.k = sh.k, c.N = sh.N;
  c.level_bsk = sh.level_bsk, c.base_log_bsk = sh.base_log_bsk;
  c.level_pksk = sh.level_pksk, c.base_log_pksk = sh.base_log_pksk;
  c.level_cbs = sh.level_cbs, c.base_log_cbs = sh.base_log_cbs;
  c.t = t, c.tau = tau, c.batch = batch;
  c.scratch = scratch, c.scratch_bytes = scratch_bytes;
  return c;
}

static int wop_run(const WopCall& c) {
  // ---- validation: nothing below this block runs, and no HIP call is made, on a refused call ----
  if (c.batch == 0) return 0;
  const bool stage1 = c.num_inputs > 0;
  if (!c.lwe_out || !c.lwe_in || !c.luts || !c.fbsk || !c.fpksk || (stage1 && !c.ksk)) {
    set_error("%s: null pointer", c.who);
    return -1;
  }
  if (c.t == 0 || c.tau == 0 || c.cbs_delta_log > 63) {
    set_error("%s: inputs=%u and luts=%u must be positive, cbs_delta_log=%u at most 63", c.who, c.t, c.tau,
              c.cbs_delta_log);
    return -3;
  }
  if (!wop_params_ok(stage1, c.n, c.k, c.N, c.level_bsk, c.base_log_bsk, c.level_ksk, c.base_log_ksk, c.level_pksk,
                     c.base_log_pksk, c.level_cbs, c.base_log_cbs)) {
    set_error("%s: unsupported parameters n=%u k=%u N=%u bsk level=%u base_log=%u, ksk level=%u base_log=%u, pksk "
              "level=%u base_log=%u, cbs level=%u base_log=%u",
              c.who, c.n, c.k, c.N, c.level_bsk, c.base_log_bsk, c.level_ksk, c.base_log_ksk, c.level_pksk,
              c.base_log_pksk, c.level_cbs, c.base_log_cbs);
    return -2;
  }
  const WopLayout lay = wop_layout(c.n, c.k, c.N, c.level_cbs, c.num_inputs, c.t, c.tau, c.batch);
  if (!lay.ok) {
    set_error("%s: inputs=%u (at most log2 N + %u) luts=%u lookups=%u overflow the call's sizes", c.who, c.t,
              WOP_MAX_R, c.tau, c.batch);
    return -3;
  }
  if (const int rc = scratch_refused(c.who, c.scratch, c.scratch_bytes, lay.bytes)) return rc;

  // ---- stage 1's per-row parameters (host) ----
  const uint64_t W = (uint64_t)c.k * c.N + 1;
  const uint64_t rows_in = (uint64_t)c.batch * c.num_inputs;
  std::vector<uint32_t> nbs(rows_in), dls(rows_in);
  std::vector<uint64_t> offs(rows_in);
  if (stage1) {
    std::vector<uint64_t> first(c.num_inputs);  // first output row of input i inside a value's t rows
    uint64_t at = 0;
    for (uint32_t q = 0; q < c.num_inputs; ++q) {
      const uint32_t i = c.msb_last ? c.num_inputs - 1 - q : q;
      first[i] = at, at += c.nb[i];
    }
    for (uint64_t b = 0; b < c.batch; ++b)
      for (uint32_t i = 0; i < c.num_inputs; ++i) {
        const uint64_t row = b * c.num_inputs + i;
        nbs[row] = c.nb[i], dls[row] = c.dl[i], offs[row] = b * c.t + first[i];
      }
  }

  const DeviceScope dev((int)c.gpu);
  hipStream_t s = (hipStream_t)c.stream;
  const CallScratch own(c.scratch, lay.bytes, s);
  char* base = own.base;
  uint64_t* d_front = (uint64_t*)(base + lay.front);
  uint64_t* d_bits = (uint64_t*)(base + lay.bits);
  uint64_t* d_ggsw = (uint64_t*)(base + lay.ggsw);
  uint64_t* d_lut = (uint64_t*)(base + lay.lut);
  void* d_stage = base + lay.stage;

  // ---- stage 1 ----
  const uint64_t* bits_in = c.lwe_in;
  if (stage1) {
    const uint64_t* eb_in = c.lwe_in;
    if (c.offsets) {
      WopOffsets off{};
      std::copy(c.offsets, c.offsets + c.num_inputs, off.v);
      const uint64_t total = rows_in * W;
      hipLaunchKernelGGL(wop_front_kernel, dim3(wop_blocks(total)), dim3(256), 0, s, d_front, c.lwe_in, off,
                         c.num_inputs, W, total);
      if (const int rc = launch_refused(c.who, "wop_front_kernel")) return rc;
      eb_in = d_front;
    }
    if (const int rc = concrete_hip_extract_bits(c.stream, c.gpu, d_bits, eb_in, c.fbsk, c.ksk, nbs.data(), dls.data(),
                                                 offs.data(), (uint32_t)(W - 1), c.n, c.k, c.N, c.base_log_bsk,
                                                 c.level_bsk, c.base_log_ksk, c.level_ksk, (uint32_t)rows_in, d_stage,
                                                 lay.stage_bytes))
      return rc;
    bits_in = d_bits;
  }

  // ---- stage 2 ----
  if (const int rc = concrete_hip_circuit_bootstrap(c.stream, c.gpu, d_ggsw, bits_in, c.fbsk, c.fpksk, c.cbs_delta_log,
                                                    c.n, c.k, c.N, c.level_bsk, c.base_log_bsk, c.level_pksk,
                                                    c.base_log_pksk, c.level_cbs, c.base_log_cbs, c.batch * c.t,
                                                    d_stage, lay.stage_bytes, nullptr))
    return rc;

  // ---- stage 3 ----
  const uint64_t* lut = c.luts;
  if (lay.r == 0 && !c.lut_padded && (1ull << c.t) < c.N) {
    const uint64_t total = (uint64_t)c.tau * c.N;
    hipLaunchKernelGGL(wop_lut_pad_kernel, dim3(wop_blocks(total)), dim3(256), 0, s, d_lut, c.luts, 1ull << c.t,
                       (uint64_t)c.N, total);
    if (const int rc = launch_refused(c.who, "wop_lut_pad_kernel")) return rc;
    lut = d_lut;
  }
  return concrete_hip_vertical_packing(c.stream, c.gpu, c.lwe_out, nullptr, d_ggsw, lut, c.k, c.N, c.base_log_cbs,
                                       c.level_cbs, lay.r, lay.m, c.tau, c.batch, d_stage, lay.stage_bytes, nullptr,
                                       c.spectrum);
}

static ScratchRegistry g_cbvp_scratch;  // scratch_cuda_circuit_bootstrap_vertical_packing_64's buffers
static ScratchRegistry g_wop_scratch;   // scratch_cuda_wop_pbs_64's

static const void* resolve_bsk(const void* fourier_bsk) {
  // a `dest` of cuda_convert_lwe_programmable_bootstrap_key_64 stands for its registered Fourier key;
  // any other pointer is a caller-owned Fourier key
  const void* f = fourier_bsk ? concrete_hip_lookup_bsk(fourier_bsk) : nullptr;
  return f ? f : fourier_bsk;
}

static void wop_scratch(const char* what, ScratchRegistry& reg, void* stream, uint32_t gpu_index, int8_t** buffer,
                        uint64_t bytes, bool allocate) {
  if (!buffer) {
    set_error("null buffer pointer");
    die(what);
  }
  *buffer = nullptr;
  if (bytes == 0) {
    set_error("scratch: unsupported parameters or sizes");
    die(what);
  }
  if (allocate) *buffer = reg.allocate(gpu_index, bytes, stream);  // else NULL: the call takes pool scratch
}

}  // namespace chip

using namespace chip;

extern "C" {

int concrete_hip_wop_pbs_supported(uint32_t lwe_dimension, uint32_t glwe_dimension, uint32_t polynomial_size,
                                   uint32_t level_bsk, uint32_t base_log_bsk, uint32_t level_ksk, uint32_t base_log_ksk,
                                   uint32_t level_pksk, uint32_t base_log_pksk, uint32_t level_cbs,
                                   uint32_t base_log_cbs) {
  return wop_params_ok(true, lwe_dimension, glwe_dimension, polynomial_size, level_bsk, base_log_bsk, level_ksk,
                       base_log_ksk, level_pksk, base_log_pksk, level_cbs, base_log_cbs)
             ? 1
             : 0;
}

uint64_t concrete_hip_wop_pbs_scratch_bytes(uint32_t lwe_dimension, uint32_t glwe_dimension, uint32_t polynomial_size,
                                            uint32_t level_cbs, uint32_t num_blocks, uint32_t number_of_bits,
                                            uint32_t tau, uint32_t batch) {
  const WopLayout l = wop_layout(lwe_dimension, glwe_dimension, polynomial_size, level_cbs, num_blocks, number_of_bits,
                                 tau, batch);
  return l.ok ? l.bytes : 0;
}

int concrete_hip_circuit_bootstrap_vertical_packing(
    void* stream, uint32_t gpu_index, uint64_t* lwe_array_out, const uint64_t* lwe_array_in,
    const uint64_t* cleartext_luts, const void* fourier_bsk, const uint64_t* fp_ksk, uint32_t lwe_dimension,
    uint32_t glwe_dimension, uint32_t polynomial_size, uint32_t level_bsk, uint32_t base_log_bsk, uint32_t level_pksk,
    uint32_t base_log_pksk, uint32_t level_cbs, uint32_t base_log_cbs, uint32_t number_of_inputs, uint32_t tau,
    uint32_t num_lookups, void* scratch, uint64_t scratch_bytes, double* ggsw_spectrum_max) {
  const WopShape sh{lwe_dimension, glwe_dimension, polynomial_size, level_bsk, base_log_bsk, level_pksk, base_log_pksk,
                    level_cbs, base_log_cbs};
  WopCall c = wop_call("circuit_bootstrap_vertical_packing", stream, gpu_index, lwe_array_out, lwe_array_in,
                       cleartext_luts, fourier_bsk, fp_ksk, sh, number_of_inputs, tau, num_lookups, scratch,
                       scratch_bytes);
  c.spectrum = ggsw_spectrum_max;
  return wop_run(c);
}

int concrete_hip_wop_pbs_crt(void* stream, uint32_t gpu_index, uint64_t* lwe_array_out, const uint64_t* lwe_array_in,
                             const uint64_t* cleartext_luts, const void* fourier_bsk, const uint64_t* ksk,
                             const uint64_t* fp_ksk, const uint64_t* moduli, uint32_t num_blocks, uint32_t batch,
                             uint32_t lwe_dimension, uint32_t glwe_dimension, uint32_t polynomial_size,
                             uint32_t level_bsk, uint32_t base_log_bsk, uint32_t level_ksk, uint32_t base_log_ksk,
                             uint32_t level_pksk, uint32_t base_log_pksk, uint32_t level_cbs, uint32_t base_log_cbs,
                             void* scratch, uint64_t scratch_bytes, double* ggsw_spectrum_max) {
  const char* who = "wop_pbs_crt";
  if (batch == 0) return 0;
  if (!moduli) {
    set_error("%s: null pointer", who);
    return -1;
  }
  if (num_blocks == 0 || num_blocks > WOP_MAX_BLOCKS) {
    set_error("%s: num_blocks=%u (1 .. %u)", who, num_blocks, WOP_MAX_BLOCKS);
    return -3;
  }
  uint32_t nb[WOP_MAX_BLOCKS], dl[WOP_MAX_BLOCKS], t = 0;
  uint64_t off[WOP_MAX_BLOCKS];
  for (uint32_t i = 0; i < num_blocks; ++i) {
    if (moduli[i] < 2 || moduli[i] > (1ull << 63)) {
      set_error("%s: modulus %u is %llu (2 .. 2^63)", who, i, (unsigned long long)moduli[i]);
      return -3;
    }
    nb[i] = crt_bits(moduli[i]), dl[i] = 64 - nb[i], t += nb[i];
    off[i] = (1ull << (63 - nb[i])) - (nb[i] <= 59 ? 1ull << (59 - nb[i]) : 0ull);
  }
  const WopShape sh{lwe_dimension, glwe_dimension, polynomial_size, level_bsk, base_log_bsk, level_pksk, base_log_pksk,
                    level_cbs, base_log_cbs};
  WopCall c = wop_call(who, stream, gpu_index, lwe_array_out, lwe_array_in, cleartext_luts, fourier_bsk, fp_ksk, sh, t,
                       num_blocks, batch, scratch, scratch_bytes);
  c.ksk = ksk, c.level_ksk = level_ksk, c.base_log_ksk = base_log_ksk;
  c.num_inputs = num_blocks, c.nb = nb, c.dl = dl, c.offsets = off, c.msb_last = true;
  c.spectrum = ggsw_spectrum_max;
  return wop_run(c);
}

void scratch_cuda_circuit_bootstrap_vertical_packing_64(void* stream, uint32_t gpu_index, int8_t** cbs_vp_buffer,
                                                        uint32_t* cbs_delta_log, uint32_t glwe_dimension,
                                                        uint32_t lwe_dimension, uint32_t polynomial_size,
                                                        uint32_t level_count_cbs, uint32_t number_of_inputs,
                                                        uint32_t lut_number, uint32_t max_shared_memory,
                                                        bool allocate_gpu_memory) {
  (void)max_shared_memory;
  if (cbs_delta_log) *cbs_delta_log = 63;
  wop_scratch("scratch_cuda_circuit_bootstrap_vertical_packing_64", g_cbvp_scratch, stream, gpu_index, cbs_vp_buffer,
              concrete_hip_wop_pbs_scratch_bytes(lwe_dimension, glwe_dimension, polynomial_size, level_count_cbs, 0,
                                                 number_of_inputs, lut_number, 1),
              allocate_gpu_memory);
}

void cuda_circuit_bootstrap_vertical_packing_64(void* stream, uint32_t gpu_index, void* lwe_array_out,
                                                const void* lwe_array_in, const void* fourier_bsk,
                                                const void* cbs_fpksk, const void* lut_vector, int8_t* cbs_vp_buffer,
                                                uint32_t cbs_delta_log, uint32_t polynomial_size,
                                                uint32_t glwe_dimension, uint32_t lwe_dimension,
                                                uint32_t level_count_bsk, uint32_t base_log_bsk,
                                                uint32_t level_count_pksk, uint32_t base_log_pksk,
                                                uint32_t level_count_cbs, uint32_t base_log_cbs,
                                                uint32_t number_of_inputs, uint32_t lut_number,
                                                uint32_t max_shared_memory) {
  (void)max_shared_memory;
  const char* what = "cuda_circuit_bootstrap_vertical_packing_64";
  const uint64_t bytes = g_cbvp_scratch.size_of(what, "scratch_cuda_circuit_bootstrap_vertical_packing_64", cbs_vp_buffer);
  const WopShape sh{lwe_dimension, glwe_dimension, polynomial_size, level_count_bsk, base_log_bsk, level_count_pksk,
                    base_log_pksk, level_count_cbs, base_log_cbs};
  WopCall c = wop_call(what, stream, gpu_index, lwe_array_out, lwe_array_in, lut_vector, resolve_bsk(fourier_bsk),
                       cbs_fpksk, sh, number_of_inputs, lut_number, 1, cbs_vp_buffer, bytes);
  c.cbs_delta_log = cbs_delta_log, c.lut_padded = true;
  if (wop_run(c) != 0) die(what);
}

void cleanup_cuda_circuit_bootstrap_vertical_packing(void* stream, uint32_t gpu_index, int8_t** cbs_vp_buffer) {
  g_cbvp_scratch.release(gpu_index, cbs_vp_buffer, stream);
}

void scratch_cuda_wop_pbs_64(void* stream, uint32_t gpu_index, int8_t** wop_pbs_buffer, uint32_t* delta_log,
                             uint32_t* cbs_delta_log, uint32_t glwe_dimension, uint32_t lwe_dimension,
                             uint32_t polynomial_size, uint32_t level_count_cbs, uint32_t level_count_bsk,
                             uint32_t number_of_bits_of_message_including_padding, uint32_t number_of_bits_to_extract,
                             uint32_t number_of_inputs, uint32_t max_shared_memory, bool allocate_gpu_memory) {
  (void)max_shared_memory, (void)level_count_bsk;
  const char* what = "scratch_cuda_wop_pbs_64";
  if (number_of_bits_of_message_including_padding == 0 || number_of_bits_of_message_including_padding > 63 ||
      (uint64_t)number_of_inputs * number_of_bits_to_extract > 0xffffffffull) {
    set_error("number_of_bits_of_message_including_padding=%u (1 .. 63), inputs=%u x bits=%u",
              number_of_bits_of_message_including_padding, number_of_inputs, number_of_bits_to_extract);
    die(what);
  }
  if (delta_log) *delta_log = 64 - number_of_bits_of_message_including_padding;
  if (cbs_delta_log) *cbs_delta_log = 63;
  wop_scratch(what, g_wop_scratch, stream, gpu_index, wop_pbs_buffer,
              concrete_hip_wop_pbs_scratch_bytes(lwe_dimension, glwe_dimension, polynomial_size, level_count_cbs,
                                                 number_of_inputs, number_of_inputs * number_of_bits_to_extract,
                                                 number_of_inputs, 1),
              allocate_gpu_memory);
}

void cuda_wop_pbs_64(void* stream, uint32_t gpu_index, void* lwe_array_out, const void* lwe_array_in,
                     const void* lut_vector, const void* fourier_bsk, const void* ksk, const void* cbs_fpksk,
                     int8_t* wop_pbs_buffer, uint32_t cbs_delta_log, uint32_t glwe_dimension, uint32_t lwe_dimension,
                     uint32_t polynomial_size, uint32_t base_log_bsk, uint32_t level_count_bsk, uint32_t base_log_ksk,
                     uint32_t level_count_ksk, uint32_t base_log_pksk, uint32_t level_count_pksk, uint32_t base_log_cbs,
                     uint32_t level_count_cbs, uint32_t number_of_bits_of_message_including_padding,
                     uint32_t number_of_bits_to_extract, uint32_t delta_log, uint32_t number_of_inputs,
                     uint32_t max_shared_memory) {
  (void)max_shared_memory, (void)number_of_bits_of_message_including_padding;
  const char* what = "cuda_wop_pbs_64";
  const uint64_t bytes = g_wop_scratch.size_of(what, "scratch_cuda_wop_pbs_64", wop_pbs_buffer);
  // the extracted bits sit at 2^63 (cuda_extract_bits_64), so that is where stage 2 must read them
  if (number_of_inputs == 0 || number_of_inputs > WOP_MAX_BLOCKS || number_of_bits_to_extract == 0 || delta_log == 0 ||
      (uint64_t)delta_log + number_of_bits_to_extract > 64 || cbs_delta_log != 63) {
    set_error("inputs=%u (1 .. %u), bits=%u at delta_log=%u (bits >= 1, delta_log >= 1, their sum at most 64), "
              "cbs_delta_log=%u (63)",
              number_of_inputs, WOP_MAX_BLOCKS, number_of_bits_to_extract, delta_log, cbs_delta_log);
    die(what);
  }
  uint32_t nb[WOP_MAX_BLOCKS], dl[WOP_MAX_BLOCKS];
  std::fill(nb, nb + number_of_inputs, number_of_bits_to_extract);
  std::fill(dl, dl + number_of_inputs, delta_log);
  const WopShape sh{lwe_dimension, glwe_dimension, polynomial_size, level_count_bsk, base_log_bsk, level_count_pksk,
                    base_log_pksk, level_count_cbs, base_log_cbs};
  WopCall c = wop_call(what, stream, gpu_index, lwe_array_out, lwe_array_in, lut_vector, resolve_bsk(fourier_bsk),
                       cbs_fpksk, sh, number_of_inputs * number_of_bits_to_extract, number_of_inputs, 1, wop_pbs_buffer,
                       bytes);
  c.ksk = (const uint64_t*)ksk, c.level_ksk = level_count_ksk, c.base_log_ksk = base_log_ksk;
  c.num_inputs = number_of_inputs, c.nb = nb, c.dl = dl;  // input 0 supplies the most significant bits
  c.lut_padded = true;
  if (wop_run(c) != 0) die(what);
}

void cleanup_cuda_wop_pbs(void* stream, uint32_t gpu_index, int8_t** wop_pbs_buffer) {
  g_wop_scratch.release(gpu_index, wop_pbs_buffer, stream);
}

}  // extern "C"
