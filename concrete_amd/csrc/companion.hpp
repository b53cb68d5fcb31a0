// companion.hpp — host side of libconcrete_hip: what the entry points share and the kernels never see.
//
// General-format companion keys.  A PBS whose digits are wider than the hand-tuned kernel of its
// (k, N, l) accepts (N = 1024: the gate (k+1) l 2^logB <= 4096, pbs.hpp pbs1024_exact; N = 2048:
// logB <= 24) but which the general path (pbs_generic.hip) runs exactly runs there, on a companion key
// in the general format built from the standard key (abi.hip generic_companion_key;
// concrete_hip_pbs_generic for caller-held keys).
//
// Host services of the key path and the ABI plumbing: the standard key's size, the
// pool switch, the current-device scope, the scratch_cuda_* registries and a call's own scratch, the
// per-key spectrum gate.  Kept apart from pbs.hpp, whose contents are the kernels' geometry.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include <mutex>
#include <unordered_map>

#include "common.hpp"
#include "pbs.hpp"

namespace chip {

KeyFormat generic_key_format(uint32_t k, uint32_t N, uint32_t level);  // pbs_generic.hip: any shape it runs

// A hand-tuned shape at digits its kernel refuses but the general path runs exactly.
inline bool pbs_needs_generic_key(uint32_t k, uint32_t N, uint32_t level, uint32_t base_log) {
  const KeyKind kind = key_format(k, N, level).kind;
  return kind != KeyKind::NONE && kind != KeyKind::GENERIC && !pbs_params_ok(k, N, level, base_log) &&
         generic_pbs_ok(k, N, level, base_log);
}

// Size in bytes of a standard-domain key ([n][l][k+1][k+1][N] u64).
inline uint64_t std_bsk_bytes(uint32_t n, uint32_t k, uint32_t level, uint32_t N) {
  return (uint64_t)n * level * ((uint64_t)k + 1) * ((uint64_t)k + 1) * N * 8ull;
}

// Size in bytes of a general-format key ([n][col][limb][row][q][N/2] complex f64).
inline uint64_t generic_fourier_bsk_bytes(uint32_t n, uint32_t k, uint32_t level, uint32_t N) {
  const KeyFormat f = generic_key_format(k, N, level);
  return f.kind == KeyKind::GENERIC ? (uint64_t)n * level * (k + 1) * (k + 1) * f.limbs * (N / 2) * 16ull : 0;
}

// abi.hip: companions of hand-tuned-format keys.  `src` is the standard key (host or device
// memory) and must outlive the registration.
void register_std_source(const void* primary, const uint64_t* src, bool on_device, uint32_t gpu, uint32_t n,
                         uint32_t k, uint32_t level, uint32_t N);
void release_std_source(const void* primary);
const void* generic_companion_key(const void* primary, uint32_t n, uint32_t k, uint32_t level, uint32_t N,
                                  hipStream_t s);

// abi.hip: the gates and the key choice of concrete_hip_pbs, for callers that launch several PBS on one
// key (extract_bits.hip).  0, or the refusal's code with the message set; makes gpu_index current.
// `generic`: launch with pbs_generic_launch on `key` (the companion), else pbs_launch.
struct PbsKey {
  const void* key;
  uint32_t limbs;
  bool generic;
};
int pbs_resolve_key(void* stream, uint32_t gpu_index, const void* fourier_bsk, uint32_t lwe_dimension,
                    uint32_t glwe_dimension, uint32_t polynomial_size, uint32_t base_log, uint32_t level_count,
                    PbsKey* out);

// keycheck.hip: the exactness gate against the converted key's measured spectrum (round 6).
// key_spectrum_record reads the max|G| the conversion kernels left in the sink (synchronises s),
// records it for `dest`, and returns -2 when no base_log could use the key exactly; key_bound_check returns -2
// (message set) when the PBS on `key` at logB would not be certified exact (0 without a record).
unsigned long long* key_spectrum_sink(hipStream_t s);  // zeroed sink for ConvertArgs::smax
int key_spectrum_record(hipStream_t s, const void* dest, const KeyFormat& f, uint32_t n, uint32_t k, uint32_t N,
                        uint32_t level, unsigned long long* sink);
int key_bound_check(const void* key, KeyKind kind, uint32_t k, uint32_t N, uint32_t level, uint32_t logB);
void key_spectrum_copy(const void* dest, const void* src);
void key_spectrum_forget(const void* key);


// abi.hip: raises the current device's default pool's release threshold to "never" (see there); called
// before every stream-ordered allocation.
void keep_pool_memory();

// abi.hip: the library's stream-ordered allocation (keep_pool_memory, hipMallocAsync, scratch_fill); the
// allocation's status.  scratch_fill: a no-op unless the test hook CONCRETE_HIP_SCRATCH_FILL names a
// byte, then the block is set to it on s before the call's kernels run.
hipError_t pool_alloc(void** p, size_t bytes, hipStream_t s);
void scratch_fill(void* p, size_t bytes, hipStream_t s);

// abi.hip: the cuda_* entry points' failure, as the reference's: the message on stderr, then abort.
[[noreturn]] void die(const char* what);

// Makes `gpu` current for a scope and restores the caller's current device on exit (torch shares it).
struct DeviceScope {
  int prev = 0;
  explicit DeviceScope(int gpu) {
    CHIP_CHECK(hipGetDevice(&prev));
    CHIP_CHECK(hipSetDevice(gpu));
  }
  ~DeviceScope() { CHIP_CHECK(hipSetDevice(prev)); }
  DeviceScope(const DeviceScope&) = delete;
  DeviceScope& operator=(const DeviceScope&) = delete;
};

// abi.hip: the buffers a family of scratch_cuda_* calls handed out, with their sizes (the calls that
// use them carry none).  One instance per family: a buffer of another family is refused.
class ScratchRegistry {
 public:
  // `bytes` from gpu's pool on s, remembered
  int8_t* allocate(uint32_t gpu, uint64_t bytes, void* stream);
  // 0 for NULL (the call takes pool scratch), else the buffer's size; dies in `what` when the
  // buffer does not come from `origin`
  uint64_t size_of(const char* what, const char* origin, const void* buffer);
  // forgets and frees *buffer on s and nulls it; a no-op on NULL
  void release(uint32_t gpu, int8_t** buffer, void* stream);

 private:
  std::mutex mu_;
  std::unordered_map<const void*, uint64_t> bytes_;
};

// A call's scratch: the caller's, or pool scratch of the call's own.  scratch_refused touches no device:
// 0, or -3 with the message set when the caller's buffer is smaller than `need` or not 16-byte aligned.
int scratch_refused(const char* who, const void* scratch, uint64_t scratch_bytes, uint64_t need);
struct CallScratch {
  char* base;
  CallScratch(void* callers, uint64_t bytes, hipStream_t s) : base((char*)callers), s_(s), owned_(!callers) {
    if (!owned_) return;
    CHIP_CHECK(pool_alloc((void**)&base, bytes, s_));
  }
  ~CallScratch() {  // on every return path; a failed CHIP_CHECK does not return at all (hip_fatal aborts)
    if (owned_) CHIP_CHECK(hipFreeAsync(base, s_));
  }
  CallScratch(const CallScratch&) = delete;
  CallScratch& operator=(const CallScratch&) = delete;

 private:
  hipStream_t s_;
  bool owned_;
};

}  // namespace chip
