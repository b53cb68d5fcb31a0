// vertical_packing.hpp — launch descriptors of the vertical packing's device code (gen_cmux_kernel and
// the natural-order GGSW conversion, pbs_generic.hip) for its host side (vertical_packing.hip).
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

namespace chip {

// What a launch of gen_cmux_kernel takes for c0 and c1 of dst = c0 + G [x] (c1 - c0):
//   LEAF    trivial GLWEs of two LUT polynomials (tree layer 0; only the body row is decomposed)
//   PAIR    two nodes of the previous layer
//   ROTATE  c1 = X^(-rot) c0 (a blind-rotation step)
enum class CmuxMode { LEAF, PAIR, ROTATE };

struct CmuxArgs {
  hipStream_t stream;
  uint64_t* dst;        // [count][(k+1) N]
  const uint64_t* src;  // PAIR: [2 count][(k+1) N], CMUX x reads nodes 2x and 2x + 1; ROTATE: [count][(k+1) N];
                        // LEAF: LUT polynomials [2 per_lookup][N], shared by the lookups
  const void* keys;     // general-format GGSWs, natural frequency order, [lookups][key_stride]
  uint32_t k, N, level, base_log;
  uint32_t count;       // CMUXes of this launch = lookups * per_lookup
  uint32_t per_lookup;  // CMUXes per lookup (tau * nodes of the layer)
  uint32_t key_stride;  // GGSWs per lookup (r + mbr_size)
  uint32_t key_index;   // this layer's GGSW within the lookup
  uint32_t rot;         // ROTATE: the monomial degree d
  unsigned long long* resid;  // optional: max |x - round(x)| (f64 bits), as PbsArgs::resid
};

// Whether gen_cmux_kernel is instantiated for the shape and the general path's gate accepts it.
bool vp_params_ok(uint32_t k, uint32_t N, uint32_t level, uint32_t base_log);
// 0, or -1 / -2 with the message set.
int vp_cmux_launch(CmuxMode mode, const CmuxArgs& a);
// `ggsws` standard GGSWs ([level][k+1][k+1][N] each, on the device) into the general key format with
// frequencies in natural order for every N; smax: keycheck.hpp sink.
int vp_convert_launch(hipStream_t s, void* dest, const uint64_t* src_dev, uint64_t ggsws, uint32_t k, uint32_t N,
                      uint32_t level, unsigned long long* smax);
// sample extraction of `count` GLWEs in coefficient order into rows of kN + 1 words
int vp_extract_launch(hipStream_t s, uint64_t* out, const uint64_t* glwes, uint32_t count, uint32_t k, uint32_t N);

}  // namespace chip
