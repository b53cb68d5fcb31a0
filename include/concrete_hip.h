/*
 * concrete_hip.h — C ABI of libconcrete_hip.so, the MI355X-native (gfx950) backend for the
 * batched programmable-bootstrap path of the Concrete compiler runtime.
 *
 * Part 1 (cuda_* / scratch_* / cleanup_* names) is exactly the set of backend entry points
 * libConcretelangRuntime calls when built with CONCRETELANG_CUDA_SUPPORT; the names are kept
 * because the runtime's compiled call sites use them.  Each declaration cites the reference
 * call site it replaces (paths relative to /root/reference/compilers/concrete-compiler/compiler).
 * Conventions: void returns, failures abort (reference `nounwind`,
 * backends/concrete-cpu/implementation/src/c_api.rs:22-36); everything is stream-ordered;
 * the caller synchronises.  `stream` is a hipStream_t created by cuda_create_stream.
 *
 * Part 2 (concrete_hip_*) are extensions: a size query for the device key format (fixes the
 * runtime's `len * sizeof(double)` allocation hazard, include/concretelang/Runtime/context.h:101-105),
 * status-returning variants, and the direct (no key registry) PBS used by the multi-GPU glue.
 */
#ifndef CONCRETE_HIP_H
#define CONCRETE_HIP_H

#include <stdbool.h>
#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

/* ------------------------------------------------------------------------------------------
 * Part 1: runtime-facing ABI (tfhe-cuda-backend names)
 * ------------------------------------------------------------------------------------------ */

/* lib/Runtime/wrappers.cpp:129,185,283; lib/Runtime/GPUDFG.cpp:191 */
void *cuda_create_stream(uint32_t gpu_index);
/* lib/Runtime/wrappers.cpp:160,255,362; lib/Runtime/GPUDFG.cpp:168 */
void cuda_destroy_stream(void *stream, uint32_t gpu_index);
/* lib/Runtime/wrappers.cpp:50,146,194; include/concretelang/Runtime/context.h:103-104 */
void *cuda_malloc_async(uint64_t size, void *stream, uint32_t gpu_index);
/* lib/Runtime/wrappers.cpp:51,222; lib/Runtime/GPUDFG.cpp:475,1194; context.h:137-139 */
void cuda_memcpy_async_to_gpu(void *dest, void *src, uint64_t size, void *stream, uint32_t gpu_index);
/* lib/Runtime/wrappers.cpp:59; lib/Runtime/GPUDFG.cpp:407,463,1034 */
void cuda_memcpy_async_to_cpu(void *dest, const void *src, uint64_t size, void *stream, uint32_t gpu_index);
/* lib/Runtime/wrappers.cpp:65,157-159; include/concretelang/Runtime/context.h:47-55 */
void cuda_drop(void *ptr, uint32_t gpu_index);
/* lib/Runtime/wrappers.cpp:246-250; lib/Runtime/GPUDFG.cpp:392,422,432,1102 */
void cuda_drop_async(void *ptr, void *stream, uint32_t gpu_index);
/* lib/Runtime/wrappers.cpp:155 */
void cuda_synchronize_device(uint32_t gpu_index);

/* include/concretelang/Runtime/context.h:104-109: H2D + conversion of the standard u64 BSK
 * (host pointer `src`, layout [n][l][k+1][k+1][N], concrete-cpu bootstrap.rs:417-429) into the
 * device key format.  `dest` is the caller's allocation of n*l*(k+1)^2*N*8 bytes; the device
 * format is larger (exact limbs), so the backend keeps it in a registry keyed by `dest` and
 * releases it when cuda_drop(dest) is called.  The key is usable once the stream is synced. */
void cuda_convert_lwe_programmable_bootstrap_key_64(void *stream, uint32_t gpu_index, void *dest, void *src,
                                                    uint32_t input_lwe_dim, uint32_t glwe_dim,
                                                    uint32_t level_count, uint32_t polynomial_size);

/* lib/Runtime/wrappers.cpp:234,341; lib/Runtime/GPUDFG.cpp:126 */
void scratch_cuda_programmable_bootstrap_64(void *stream, uint32_t gpu_index, int8_t **pbs_buffer,
                                            uint32_t glwe_dimension, uint32_t polynomial_size,
                                            uint32_t level_count, uint32_t input_lwe_ciphertext_count,
                                            bool allocate_gpu_memory);
/* lib/Runtime/wrappers.cpp:241,348; lib/Runtime/GPUDFG.cpp:131 */
void cleanup_cuda_programmable_bootstrap(void *stream, uint32_t gpu_index, int8_t **pbs_buffer);

/* lib/Runtime/wrappers.cpp:237-240,344-347; lib/Runtime/GPUDFG.cpp:1214-1218: batched classic PBS.
 *   out[out_idx[s]] (kN+1 u64) = PBS(in[in_idx[s]] (n+1 u64), lut_vector[lut_idx[s]] ((k+1)N u64))
 * bootstrapping_key is the `dest` of cuda_convert_lwe_programmable_bootstrap_key_64.
 * The last two arguments are passed as (1, 1) by every reference call site (one LUT per
 * sample, stride 1); other values abort. */
void cuda_programmable_bootstrap_lwe_ciphertext_vector_64(
    void *stream, uint32_t gpu_index, void *lwe_array_out, void *lwe_output_indexes, void *lut_vector,
    void *lut_vector_indexes, void *lwe_array_in, void *lwe_input_indexes, void *bootstrapping_key,
    int8_t *pbs_buffer, uint32_t lwe_dimension, uint32_t glwe_dimension, uint32_t polynomial_size,
    uint32_t base_log, uint32_t level_count, uint32_t num_samples, uint32_t num_many_lut, uint32_t lut_stride);

/* lib/Runtime/wrappers.cpp:149-151, GPUDFG.cpp:1098-1101: batched LWE keyswitch; ksk is the
 * standard u64 key [n_in][l][n_out+1] copied verbatim to the device (context.h:117-145).
 * Exact u64 result.  For base_log <= 7 and >= 64 samples it runs on the int8 matrix cores
 * (key words split into bytes, exact int32 sums) with stream-ordered scratch: the key bytes
 * (8 (n_out+1) n_in l B) and the batch's int8 digits (<= 1 GiB per pass). */
void cuda_keyswitch_lwe_ciphertext_vector_64(void *stream, uint32_t gpu_index, void *lwe_array_out,
                                             void *lwe_output_indexes, void *lwe_array_in,
                                             void *lwe_input_indexes, void *ksk, uint32_t lwe_dimension_in,
                                             uint32_t lwe_dimension_out, uint32_t base_log,
                                             uint32_t level_count, uint32_t num_samples);

/* The four linear-operation vectors of the dataflow route (GPUDFG.cpp:1286-1289, 1344-1346,
 * 1402-1404, 1445-1446): batch-major (count, lwe_dimension + 1) u64 ciphertexts, wrapping.
 * plaintext/cleartext arrays hold one u64 per ciphertext. */
void cuda_add_lwe_ciphertext_vector_64(void *stream, uint32_t gpu_index, void *lwe_array_out,
                                       const void *lwe_array_in_1, const void *lwe_array_in_2,
                                       uint32_t input_lwe_dimension, uint32_t input_lwe_ciphertext_count);
void cuda_add_lwe_ciphertext_vector_plaintext_vector_64(void *stream, uint32_t gpu_index, void *lwe_array_out,
                                                        const void *lwe_array_in, const void *plaintext_array_in,
                                                        uint32_t input_lwe_dimension,
                                                        uint32_t input_lwe_ciphertext_count);
void cuda_mult_lwe_ciphertext_vector_cleartext_vector_64(void *stream, uint32_t gpu_index, void *lwe_array_out,
                                                         const void *lwe_array_in, const void *cleartext_array_in,
                                                         uint32_t input_lwe_dimension,
                                                         uint32_t input_lwe_ciphertext_count);
void cuda_negate_lwe_ciphertext_vector_64(void *stream, uint32_t gpu_index, void *lwe_array_out,
                                          const void *lwe_array_in, uint32_t input_lwe_dimension,
                                          uint32_t input_lwe_ciphertext_count);

/* Bit extraction, stage 1 of the WoP-PBS (concrete-cuda rust_api/src/cuda_bind.rs:494-567; the CPU
 * runtime's memref_wop_pbs_crt_buffer runs the same primitive per CRT block, lib/Runtime/wrappers.cpp:
 * 934-965).  From each of number_of_samples LWE ciphertexts of dimension lwe_dimension_in = k N,
 * number_of_bits bits starting at bit delta_log are extracted, most significant first: output row
 * s * number_of_bits + j (lwe_dimension_out + 1 words) encrypts bit j of sample s times 2^63.  The input
 * is not modified.  `lwe_dimension` of the scratch call is the small dimension (lwe_dimension_out);
 * max_shared_memory is accepted and ignored.  fourier_bsk is the `dest` of
 * cuda_convert_lwe_programmable_bootstrap_key_64, or a caller-owned Fourier key
 * (concrete_hip_convert_bsk).  A scratch call with allocate_gpu_memory = false leaves NULL, and a NULL
 * buffer makes the extraction take stream-ordered pool scratch.  Bad arguments abort. */
void scratch_cuda_extract_bits_64(void *stream, uint32_t gpu_index, int8_t **bit_extract_buffer,
                                  uint32_t glwe_dimension, uint32_t lwe_dimension, uint32_t polynomial_size,
                                  uint32_t level_count, uint32_t number_of_inputs, uint32_t max_shared_memory,
                                  bool allocate_gpu_memory);
void cuda_extract_bits_64(void *stream, uint32_t gpu_index, void *list_lwe_array_out, const void *lwe_array_in,
                          int8_t *bit_extract_buffer, const void *ksk, const void *fourier_bsk,
                          uint32_t number_of_bits, uint32_t delta_log, uint32_t lwe_dimension_in,
                          uint32_t lwe_dimension_out, uint32_t glwe_dimension, uint32_t polynomial_size,
                          uint32_t base_log_bsk, uint32_t level_count_bsk, uint32_t base_log_ksk,
                          uint32_t level_count_ksk, uint32_t number_of_samples, uint32_t max_shared_memory);
void cleanup_cuda_extract_bits(void *stream, uint32_t gpu_index, int8_t **bit_extract_buffer);

/* Vertical packing, stage 3 of the WoP-PBS (concrete-cuda rust_api/src/cuda_bind.rs:369-488; DESIGN.md
 * §4.19).  ggsw_in: standard-domain GGSWs of level_count x (k+1) x (k+1) x N words each, level matrix 0
 * being decomposition level 1 (one entry of a standard bootstrapping key).
 * cuda_cmux_tree_64: `r` GGSWs, most significant bit first, select one of 2^r LUT polynomials per output;
 * lut_vector is [tau][2^r][N], glwe_array_out [tau][(k+1)N].
 * cuda_blind_rotate_and_sample_extraction_64: lut_vector holds `tau` GLWEs of (k+1)N words (what the tree
 * call wrote); GGSW j (j = mbr_size-1 down to 0) turns acc into X^(-2^(mbr_size-1-j)) acc when its bit is
 * set; lwe_out receives tau rows of kN + 1 words.
 * max_shared_memory is accepted and ignored.  A scratch call with allocate_gpu_memory = false leaves NULL,
 * and a NULL buffer makes the call take stream-ordered pool scratch.  Each call converts its GGSWs and reads
 * their largest spectrum back before it computes: ONE host synchronisation of the stream per call.  Bad
 * arguments, unsupported parameters and GGSWs that fail the exactness gate abort. */
void scratch_cuda_cmux_tree_64(void *stream, uint32_t gpu_index, int8_t **cmux_tree_buffer, uint32_t glwe_dimension,
                               uint32_t polynomial_size, uint32_t level_count, uint32_t r, uint32_t tau,
                               uint32_t max_shared_memory, bool allocate_gpu_memory);
void cuda_cmux_tree_64(void *stream, uint32_t gpu_index, void *glwe_array_out, const void *ggsw_in,
                       const void *lut_vector, int8_t *cmux_tree_buffer, uint32_t glwe_dimension,
                       uint32_t polynomial_size, uint32_t base_log, uint32_t level_count, uint32_t r, uint32_t tau,
                       uint32_t max_shared_memory);
void cleanup_cuda_cmux_tree(void *stream, uint32_t gpu_index, int8_t **cmux_tree_buffer);
void scratch_cuda_blind_rotation_sample_extraction_64(void *stream, uint32_t gpu_index, int8_t **br_se_buffer,
                                                      uint32_t glwe_dimension, uint32_t polynomial_size,
                                                      uint32_t level_count, uint32_t mbr_size, uint32_t tau,
                                                      uint32_t max_shared_memory, bool allocate_gpu_memory);
void cuda_blind_rotate_and_sample_extraction_64(void *stream, uint32_t gpu_index, void *lwe_out, const void *ggsw_in,
                                                const void *lut_vector, int8_t *br_se_buffer, uint32_t mbr_size,
                                                uint32_t tau, uint32_t glwe_dimension, uint32_t polynomial_size,
                                                uint32_t base_log, uint32_t level_count, uint32_t max_shared_memory);
void cleanup_cuda_blind_rotation_sample_extraction(void *stream, uint32_t gpu_index, int8_t **br_se_buffer);

/* Circuit bootstrap, stage 2 of the WoP-PBS, and the private functional packing keyswitch (fp-ks) it ends
 * with (concrete-cuda rust_api/src/cuda_bind.rs:334-364, 566-648).
 * fp_ksk_array: [k+1 keys][kN+1 blocks][level][(k+1)N] words; block j < kN belongs to bit j of the flattened
 * GLWE key, block kN to the constant -1; inside a block storage index t holds decomposition level `level - t`,
 * as in this header's LWE keyswitch keys (concrete_hip_fpksk_generate writes one).
 * cuda_fp_keyswitch_lwe_to_glwe_64: input row i (kN + 1 words) goes through key i mod number_of_keys and is
 * written to GLWE i of glwe_array_out ([number_of_input_lwe][(k+1)N]).  The reference's implementation is not
 * part of the sources this backend was written against; this is the reading under which the (k+1)-fold input
 * buffer its circuit bootstrap documents composes with it.
 * cuda_circuit_bootstrap_64: every input row (lwe_dimension + 1 words, the bit at delta_log) becomes one
 * standard-domain GGSW of level_cbs x (k+1) x (k+1)N words; ggsw_out is [number_of_samples][level_cbs][k+1]
 * [(k+1)N], level matrix 0 being decomposition level 1 (the order of one entry of a standard bootstrapping key
 * and of cuda_cmux_tree_64's ggsw_in; newer tfhe versions store GGSW levels reversed).  fourier_bsk is as in
 * cuda_extract_bits_64.  lut_vector_indexes: number_of_samples x level_cbs u64 entries on the device, as in
 * cuda_programmable_bootstrap_lwe_ciphertext_vector_64, entry (sample, v) naming the level (0 .. level_cbs-1)
 * whose test vector row (sample, v) uses; NULL stands for (sample, v) -> v.  `level_count` of the scratch call
 * is level_cbs.  max_shared_memory is accepted and ignored.  A scratch call with allocate_gpu_memory = false
 * leaves NULL, and a NULL buffer makes the call take stream-ordered pool scratch.  Bad arguments, unsupported
 * parameters and a key that fails the PBS exactness gate abort. */
void cuda_fp_keyswitch_lwe_to_glwe_64(void *stream, uint32_t gpu_index, void *glwe_array_out, const void *lwe_array_in,
                                      const void *fp_ksk_array, uint32_t input_lwe_dimension,
                                      uint32_t output_glwe_dimension, uint32_t output_polynomial_size,
                                      uint32_t base_log, uint32_t level_count, uint32_t number_of_input_lwe,
                                      uint32_t number_of_keys);
void scratch_cuda_circuit_bootstrap_64(void *stream, uint32_t gpu_index, int8_t **cbs_buffer, uint32_t glwe_dimension,
                                       uint32_t lwe_dimension, uint32_t polynomial_size, uint32_t level_count,
                                       uint32_t number_of_inputs, uint32_t max_shared_memory,
                                       bool allocate_gpu_memory);
void cuda_circuit_bootstrap_64(void *stream, uint32_t gpu_index, void *ggsw_out, const void *lwe_array_in,
                               const void *fourier_bsk, const void *fp_ksk_array, const void *lut_vector_indexes,
                               int8_t *cbs_buffer, uint32_t delta_log, uint32_t polynomial_size,
                               uint32_t glwe_dimension, uint32_t lwe_dimension, uint32_t level_bsk,
                               uint32_t base_log_bsk, uint32_t level_pksk, uint32_t base_log_pksk, uint32_t level_cbs,
                               uint32_t base_log_cbs, uint32_t number_of_samples, uint32_t max_shared_memory);
void cleanup_cuda_circuit_bootstrap(void *stream, uint32_t gpu_index, int8_t **cbs_buffer);

/* The WoP-PBS drivers (concrete-cuda rust_api/src/cuda_bind.rs:650-813): stages 2 and 3, and
 * all three stages, in one call.  The reference's implementation is not part of the sources this backend was
 * written against; this is the reading of its argument lists:
 * cuda_circuit_bootstrap_vertical_packing_64: lwe_array_in holds number_of_inputs bit ciphertexts (lwe_dimension
 * + 1 words each, the bit at cbs_delta_log), most significant first; they are circuit-bootstrapped (lut indexes
 * (sample, v) -> v) and select, by vertical packing at (level_count_cbs, base_log_cbs) with r = max(t - log2 N, 0)
 * tree bits and min(t, log2 N) rotation bits (t = number_of_inputs), one entry of each of the lut_number LUTs;
 * lut_vector is [lut_number][max(2^t, N)] device words (a LUT of fewer than N words sits at the front of a zero
 * polynomial); lwe_array_out receives lut_number rows of kN + 1 words.
 * cuda_wop_pbs_64: from each of the number_of_inputs inputs (kN + 1 words) number_of_bits_to_extract bits are
 * extracted at delta_log, input 0 supplying the most significant ones; ONE lookup follows with t =
 * number_of_inputs * number_of_bits_to_extract and number_of_inputs LUTs in the layout above; lwe_array_out
 * receives number_of_inputs rows of kN + 1 words.  At most 16 inputs.  cbs_delta_log must be 63, where the
 * extraction leaves its bits.
 * The scratch calls write *cbs_delta_log = 63 and *delta_log = 64 - number_of_bits_of_message_including_padding.
 * max_shared_memory is accepted and ignored.  A scratch call with allocate_gpu_memory = false leaves NULL, and a
 * NULL buffer makes the call take stream-ordered pool scratch.  fourier_bsk is as in cuda_extract_bits_64.  One
 * host synchronisation of the stream per call in the steady state (vertical packing's gate; see
 * concrete_hip_wop_pbs_crt).  Bad arguments, unsupported parameters
 * and keys or GGSWs that fail an exactness gate abort. */
void scratch_cuda_circuit_bootstrap_vertical_packing_64(void *stream, uint32_t gpu_index, int8_t **cbs_vp_buffer,
                                                        uint32_t *cbs_delta_log, uint32_t glwe_dimension,
                                                        uint32_t lwe_dimension, uint32_t polynomial_size,
                                                        uint32_t level_count_cbs, uint32_t number_of_inputs,
                                                        uint32_t lut_number, uint32_t max_shared_memory,
                                                        bool allocate_gpu_memory);
void cuda_circuit_bootstrap_vertical_packing_64(void *stream, uint32_t gpu_index, void *lwe_array_out,
                                                const void *lwe_array_in, const void *fourier_bsk,
                                                const void *cbs_fpksk, const void *lut_vector, int8_t *cbs_vp_buffer,
                                                uint32_t cbs_delta_log, uint32_t polynomial_size,
                                                uint32_t glwe_dimension, uint32_t lwe_dimension,
                                                uint32_t level_count_bsk, uint32_t base_log_bsk,
                                                uint32_t level_count_pksk, uint32_t base_log_pksk,
                                                uint32_t level_count_cbs, uint32_t base_log_cbs,
                                                uint32_t number_of_inputs, uint32_t lut_number,
                                                uint32_t max_shared_memory);
void cleanup_cuda_circuit_bootstrap_vertical_packing(void *stream, uint32_t gpu_index, int8_t **cbs_vp_buffer);
void scratch_cuda_wop_pbs_64(void *stream, uint32_t gpu_index, int8_t **wop_pbs_buffer, uint32_t *delta_log,
                             uint32_t *cbs_delta_log, uint32_t glwe_dimension, uint32_t lwe_dimension,
                             uint32_t polynomial_size, uint32_t level_count_cbs, uint32_t level_count_bsk,
                             uint32_t number_of_bits_of_message_including_padding, uint32_t number_of_bits_to_extract,
                             uint32_t number_of_inputs, uint32_t max_shared_memory, bool allocate_gpu_memory);
void cuda_wop_pbs_64(void *stream, uint32_t gpu_index, void *lwe_array_out, const void *lwe_array_in,
                     const void *lut_vector, const void *fourier_bsk, const void *ksk, const void *cbs_fpksk,
                     int8_t *wop_pbs_buffer, uint32_t cbs_delta_log, uint32_t glwe_dimension, uint32_t lwe_dimension,
                     uint32_t polynomial_size, uint32_t base_log_bsk, uint32_t level_count_bsk, uint32_t base_log_ksk,
                     uint32_t level_count_ksk, uint32_t base_log_pksk, uint32_t level_count_pksk, uint32_t base_log_cbs,
                     uint32_t level_count_cbs, uint32_t number_of_bits_of_message_including_padding,
                     uint32_t number_of_bits_to_extract, uint32_t delta_log, uint32_t number_of_inputs,
                     uint32_t max_shared_memory);
void cleanup_cuda_wop_pbs(void *stream, uint32_t gpu_index, int8_t **wop_pbs_buffer);

/* ------------------------------------------------------------------------------------------
 * Part 2: extensions (return 0 on success, < 0 on error; message via concrete_hip_last_error)
 * ------------------------------------------------------------------------------------------ */

/* ABI version of this header (2: round 3 — context-resolved memref_*_cuda_u64, stream emulator;
 * 3: round 4 — keyswitch support query, key level-order check against client keys;
 * 4: round 5 — status words per (device, stream): concrete_hip_stream_status,
 *    concrete_hip_set_thread_spin_limit;
 * 5: round 6 — status slots recycled on stream destroy (concrete_hip_status_slots_in_use,
 *    concrete_hip_set_status_slot_cap), converted keys checked against the certified bound
 *    (concrete_hip_key_spectrum_max)).
 * Bit extraction (cuda_extract_bits_64, concrete_hip_extract_bits*) was added without a new version:
 * the value stays 5, and a caller finds the capability through concrete_hip_extract_bits_supported.
 * The same holds for vertical packing (cuda_cmux_tree_64, cuda_blind_rotate_and_sample_extraction_64,
 * concrete_hip_vertical_packing*): concrete_hip_vertical_packing_supported; and for the circuit bootstrap
 * (cuda_circuit_bootstrap_64, cuda_fp_keyswitch_lwe_to_glwe_64, concrete_hip_circuit_bootstrap*,
 * concrete_hip_fp_keyswitch): concrete_hip_circuit_bootstrap_supported; and for the chained WoP-PBS
 * (cuda_circuit_bootstrap_vertical_packing_64, cuda_wop_pbs_64, concrete_hip_wop_pbs*,
 * concrete_hip_circuit_bootstrap_vertical_packing, memref_wop_pbs_crt_buffer_*): concrete_hip_wop_pbs_supported. */
uint32_t concrete_hip_abi_version(void);
/* thread-local message of the last failed concrete_hip_* call */
const char *concrete_hip_last_error(void);
/* 1 if (k, N, level, base_log) has a compiled PBS kernel (wide digits: the general path), else 0 */
int concrete_hip_pbs_supported(uint32_t glwe_dim, uint32_t polynomial_size, uint32_t level_count,
                               uint32_t base_log);
/* 1 if the batched keyswitch runs (level, base_log, n_in -> n_out): level * base_log < 64,
 * n_out + 1 <= 65536; else 0 (round 4) */
int concrete_hip_keyswitch_supported(uint32_t level_count, uint32_t base_log, uint32_t input_lwe_dim,
                                     uint32_t output_lwe_dim);
/* DEPRECATED (kept for ABI version 2 callers): number of exact key limbs of the device format for
 * k = 1 only (it takes no glwe_dim; the k-dependent formats of round 4 differ, e.g. 5 limbs at
 * k = 4, N = 512, l = 2).  Use concrete_hip_bsk_format, which takes k. */
uint32_t concrete_hip_bsk_limbs(uint32_t polynomial_size, uint32_t level_count, uint32_t base_log);
/* device key format of (k, N, l): 0 unsupported, 1 / 2 the N = 1024 / 2048 (k = 1) kernels' layouts,
 * 3 the general path (pbs_generic.hip), 4 the k = 2, N = 1024 kernels' layout (pbs1024k2.hip,
 * round 4), 5 the small-ring kernels' (N = 512, k = 3 / N = 256, k = 5, 6, l <= 3: pbs_small.hip; N = 512,
 * k = 4, any l: pbs512k4.hip; round 4); code 2 covers N = 2048, l <= 4; *limbs
 * balanced key limbs of *limb_bits bits each */
int concrete_hip_bsk_format(uint32_t glwe_dim, uint32_t polynomial_size, uint32_t level_count, uint32_t *limbs,
                            uint32_t *limb_bits);
/* rounding-error bound of the general path's exact product for a key whose largest
 * limb-spectrum magnitude is max_key_spectrum (<= 0: the random-key estimate the gate uses);
 * -1 when (k, N, l) is not on the general path */
double concrete_hip_generic_error_bound(uint32_t glwe_dim, uint32_t polynomial_size, uint32_t level_count,
                                        uint32_t base_log, double max_key_spectrum);
/* The exactness gate against the converted key (round 6).  Every conversion (concrete_hip_convert_bsk,
 * concrete_hip_convert_bsk_generic, cuda_convert_lwe_programmable_bootstrap_key_64, keyset keys and
 * general-format companions) reduces the largest limb-spectrum magnitude max|G| of the key it wrote,
 * records it with the key's device address, and returns -2 when no base_log could use the key exactly;
 * it synchronises its stream (the reference does too, context.h:110-113).  A PBS on a recorded key
 * evaluates its kernel's certified rounding bound with that max|G| at its base_log and
 * returns -2 when the bound reaches 1/2 (a hand-tuned kernel's key first falls back to the general
 * path's companion when the backend holds its standard key and the companion's bound holds).
 * concrete_hip_key_spectrum_max: the recorded max|G| of a converted key, -1 when none;
 * concrete_hip_key_error_bound: the certified bound of a PBS on that key at base_log, -1 when none. */
double concrete_hip_key_spectrum_max(const void *fourier_key);
double concrete_hip_key_error_bound(const void *fourier_key, uint32_t base_log);
/* bytes of the device (Fourier, exact-limb) bootstrapping key */
uint64_t concrete_hip_fourier_bsk_size_bytes(uint32_t input_lwe_dim, uint32_t glwe_dim, uint32_t level_count,
                                             uint32_t polynomial_size);
/* convert a standard u64 BSK (host pointer if src_is_device == 0, else device pointer) into a
 * caller-owned device buffer of concrete_hip_fourier_bsk_size_bytes() bytes */
int concrete_hip_convert_bsk(void *stream, uint32_t gpu_index, void *dest_fourier, const void *src,
                             int src_is_device, uint32_t input_lwe_dim, uint32_t glwe_dim, uint32_t level_count,
                             uint32_t polynomial_size);
/* Wide digits.  A (k, N, l) with a hand-tuned kernel (concrete_hip_bsk_format code 1, 2, 4 or 5)
 * accepts only digits that kernel keeps exact (k = 1, N = 1024: (k+1) l 2^logB <= 4096; l = 1 on the
 * 16-bit-limb kernels: logB <= 24; whole-digit levels: l 2^(logB-1) <= 2^15, or logB <= 16 on the
 * 13-bit-limb key of k = 4, N = 512, l = 2); wider ones run on the general path (pbs_generic.hip),
 * which needs the key in its own format.  Keys converted
 * through a keyset or cuda_convert_lwe_programmable_bootstrap_key_64 get that companion built from
 * their standard key on first use (concrete_hip_pbs, the memref / stream-emulator routes); a
 * caller holding its own key converts it with these two and calls concrete_hip_pbs_generic. */
uint64_t concrete_hip_generic_bsk_size_bytes(uint32_t input_lwe_dim, uint32_t glwe_dim, uint32_t level_count,
                                             uint32_t polynomial_size);
int concrete_hip_convert_bsk_generic(void *stream, uint32_t gpu_index, void *dest, const void *src,
                                     int src_is_device, uint32_t input_lwe_dim, uint32_t glwe_dim,
                                     uint32_t level_count, uint32_t polynomial_size);
int concrete_hip_pbs_generic(void *stream, uint32_t gpu_index, uint64_t *lwe_array_out,
                             const uint64_t *lwe_output_indexes, const uint64_t *lut_vector,
                             const uint64_t *lut_vector_indexes, const uint64_t *lwe_array_in,
                             const uint64_t *lwe_input_indexes, const void *generic_bsk, uint32_t lwe_dimension,
                             uint32_t glwe_dimension, uint32_t polynomial_size, uint32_t base_log,
                             uint32_t level_count, uint32_t num_samples, uint64_t *resid_bits);
/* batched PBS on a caller-owned Fourier key (no registry lookup); index arrays may be NULL
 * (identity for in/out, LUT 0 for lut).  resid_bits: optional device u64 receiving the f64
 * bits of max |x - round(x)| seen in the exact recombination (diagnostics; slower kernel). */
int concrete_hip_pbs(void *stream, uint32_t gpu_index, uint64_t *lwe_array_out, const uint64_t *lwe_output_indexes,
                     const uint64_t *lut_vector, const uint64_t *lut_vector_indexes, const uint64_t *lwe_array_in,
                     const uint64_t *lwe_input_indexes, const void *fourier_bsk, uint32_t lwe_dimension,
                     uint32_t glwe_dimension, uint32_t polynomial_size, uint32_t base_log, uint32_t level_count,
                     uint32_t num_samples, uint64_t *resid_bits);
/* batched keyswitch, status-returning variant */
int concrete_hip_keyswitch(void *stream, uint32_t gpu_index, uint64_t *lwe_array_out,
                           const uint64_t *lwe_output_indexes, const uint64_t *lwe_array_in,
                           const uint64_t *lwe_input_indexes, const uint64_t *ksk, uint32_t lwe_dimension_in,
                           uint32_t lwe_dimension_out, uint32_t base_log, uint32_t level_count,
                           uint32_t num_samples);
/* Bit extraction with a status code and per-row parameters.  number_of_bits, delta_log and
 * out_row_offsets are HOST arrays of num_samples entries; everything else that is a pointer is device
 * memory.  Row i yields number_of_bits[i] ciphertexts of dimension lwe_dimension_out, most significant
 * bit first, in output rows out_row_offsets[i] .. + number_of_bits[i] - 1 of the sum(number_of_bits)-row
 * output; out_row_offsets == NULL packs the blocks in input order.  The u64 result is bit-identical to the
 * loop of concrete_hip_keyswitch and concrete_hip_pbs it replaces.  scratch: a 16-byte aligned device
 * buffer of at least concrete_hip_extract_bits_scratch_bytes(..., max number_of_bits) bytes, or NULL for
 * stream-ordered pool scratch.  Stream-ordered; no host synchronisation between the iterations.
 * Checked before the first device call: -1 null pointer; -3 a row with number_of_bits == 0, delta_log == 0
 * or delta_log + number_of_bits > 64, lwe_dimension_in != glwe_dimension * polynomial_size, output blocks
 * that overlap or leave the output rows, a scratch buffer too small or misaligned; -2 parameters the
 * PBS or the keyswitch does not take (also: a key that fails the PBS exactness gate).  Nothing is written
 * by a refused call. */
int concrete_hip_extract_bits(void *stream, uint32_t gpu_index, uint64_t *lwe_array_out, const uint64_t *lwe_array_in,
                              const void *fourier_bsk, const uint64_t *ksk, const uint32_t *number_of_bits,
                              const uint32_t *delta_log, const uint64_t *out_row_offsets, uint32_t lwe_dimension_in,
                              uint32_t lwe_dimension_out, uint32_t glwe_dimension, uint32_t polynomial_size,
                              uint32_t base_log_bsk, uint32_t level_count_bsk, uint32_t base_log_ksk,
                              uint32_t level_count_ksk, uint32_t num_samples, void *scratch, uint64_t scratch_bytes);
/* scratch bytes of a call on num_samples rows of at most max_number_of_bits (1 .. 63) bits each; 0 for
 * num_samples == 0 or max_number_of_bits out of range.  Does not decrease with either. */
uint64_t concrete_hip_extract_bits_scratch_bytes(uint32_t lwe_dimension_in, uint32_t lwe_dimension_out,
                                                 uint32_t glwe_dimension, uint32_t polynomial_size,
                                                 uint32_t num_samples, uint32_t max_number_of_bits);
/* 1 when concrete_hip_pbs_supported(k, N, level_bsk, base_log_bsk) and concrete_hip_keyswitch_supported(
 * level_ksk, base_log_ksk, lwe_dimension_in, lwe_dimension_out) both hold and lwe_dimension_in == k N */
int concrete_hip_extract_bits_supported(uint32_t lwe_dimension_in, uint32_t lwe_dimension_out,
                                        uint32_t glwe_dimension, uint32_t polynomial_size, uint32_t base_log_bsk,
                                        uint32_t level_count_bsk, uint32_t base_log_ksk, uint32_t level_count_ksk);
/* Vertical packing with a status code, batched over num_lookups independent lookups that share the LUTs
 * (DESIGN.md §4.19).  Per lookup: a CMUX tree over the first r GGSWs (most significant bit first) picks one
 * of the 2^r LUT polynomials of each of the tau outputs; the next mbr_size GGSWs rotate the result, GGSW j
 * (j = mbr_size-1 down to 0) by X^(-2^(mbr_size-1-j)); the sample extraction of the result is written to
 * lwe_array_out.  cmux(c0, c1, G) = c0 + G [x] (c1 - c0) with the exact external product: the u64 result is
 * the integer definition's, bit for bit.  Every pointer but ggsw_spectrum_max is device memory.
 *   lwe_array_out  [num_lookups][tau][kN+1]; may be NULL only when mbr_size == 0 and glwe_tree_out is given
 *   glwe_tree_out  optional [num_lookups][tau][(k+1)N]: the tree's result
 *   ggsw_in        [num_lookups][r + mbr_size] standard-domain GGSWs of level x (k+1) x (k+1) x N words,
 *                  the tree's first (may be NULL when r + mbr_size == 0)
 *   lut_vector     [tau][2^r][N]
 *   scratch        16-byte aligned, at least concrete_hip_vertical_packing_scratch_bytes() bytes, or NULL
 *                  for stream-ordered pool scratch
 *   resid_bits     optional device u64, as concrete_hip_pbs
 *   ggsw_spectrum_max  optional HOST double: the measured max|G| of the converted GGSWs (0 without GGSWs);
 *                  also written when the gate refuses the call, left untouched by every other refusal
 * The GGSWs are converted into the general key format and gated like any converted key: the call reads
 * their largest limb-spectrum magnitude back (ONE host synchronisation of the stream per call) and returns -2
 * when the general format's certified rounding bound (the bound of the general key format of
 * (k, N, level), whatever the primary format of that shape) at that magnitude and base_log reaches 1/2.  That
 * is concrete_hip_generic_error_bound's value where that function answers; it answers -1 for a (k, N, level)
 * whose primary format is a hand-tuned kernel's, e.g. (1, 1024, 3) and (1, 2048, 2), and the gate applies
 * there all the same.  After that the call is stream-ordered: no host synchronisation, device-to-host copy
 * or allocation between the layers.
 * Checked before the first device call: -1 null lut_vector, or null ggsw_in with r + mbr_size > 0;
 * -3 tau == 0, num_lookups == 0, r > 24, mbr_size > log2 N, sizes that overflow, lwe_array_out == NULL with
 * mbr_size > 0 or without glwe_tree_out, a scratch buffer too small or misaligned; -2 parameters for which
 * concrete_hip_vertical_packing_supported is 0.  Nothing is written by a refused call. */
int concrete_hip_vertical_packing(void *stream, uint32_t gpu_index, uint64_t *lwe_array_out, uint64_t *glwe_tree_out,
                                  const uint64_t *ggsw_in, const uint64_t *lut_vector, uint32_t glwe_dimension,
                                  uint32_t polynomial_size, uint32_t base_log, uint32_t level_count, uint32_t r,
                                  uint32_t mbr_size, uint32_t tau, uint32_t num_lookups, void *scratch,
                                  uint64_t scratch_bytes, uint64_t *resid_bits, double *ggsw_spectrum_max);
/* scratch bytes of such a call; 0 for tau == 0, num_lookups == 0, r > 24, mbr_size > log2 N, a (k, N, level)
 * without a general key format, or sizes that overflow.  Does not decrease with r, tau or num_lookups. */
uint64_t concrete_hip_vertical_packing_scratch_bytes(uint32_t glwe_dimension, uint32_t polynomial_size,
                                                     uint32_t level_count, uint32_t r, uint32_t mbr_size, uint32_t tau,
                                                     uint32_t num_lookups);
/* 1 for N = 512, 1024, 2048, k <= 3 and a (level, base_log) the general path keeps exact, else 0 */
int concrete_hip_vertical_packing_supported(uint32_t glwe_dimension, uint32_t polynomial_size, uint32_t level_count,
                                            uint32_t base_log);
/* Private functional packing keyswitch with a status code: every one of num_rows LWE rows
 * (lwe_dimension_in + 1 = kN + 1 words, body last) goes through every one of the num_keys keys of fp_ksk (the
 * layout above with num_keys keys; the circuit bootstrap uses k + 1):
 *   glwe_array_out[r][i] = - sum_{j = 0 .. kN} sum_level d(x_r[j], level) * fp_ksk[i][j][level]   (mod 2^64)
 * with d the balanced signed decomposition of every word, the body included, and no body term added: the
 * library's LWE keyswitch of the row (x_r, 0) with n_in = kN + 1 and n_out + 1 = (k+1)N, word for word.
 * glwe_array_out is [num_rows][num_keys][(k+1)N].  Any (level, base_log) with level * base_log < 64.
 * Stream-ordered.  Checked before the first device call: -1 null pointer; -3 num_keys == 0,
 * lwe_dimension_in != k N, sizes that overflow; -2 parameters for which concrete_hip_keyswitch_supported(level,
 * base_log, kN + 1, (k+1)N - 1) is 0.  Nothing is written by a refused call. */
int concrete_hip_fp_keyswitch(void *stream, uint32_t gpu_index, uint64_t *glwe_array_out, const uint64_t *lwe_array_in,
                              const uint64_t *fp_ksk, uint32_t lwe_dimension_in, uint32_t glwe_dimension,
                              uint32_t polynomial_size, uint32_t base_log, uint32_t level_count, uint32_t num_rows,
                              uint32_t num_keys);
/* Circuit bootstrap with a status code.  Per input row c (lwe_dimension + 1 words) and
 * v = 0 .. level_cbs-1, level = v + 1: u = c * 2^(63 - delta_log) with 2^62 added to the body;
 * w = PBS(u, acc_v), acc_v the trivial GLWE whose body coefficients all are -(2^(63 - base_log_cbs * level));
 * w.body += 2^(63 - base_log_cbs * level); row i (0 .. k) of level matrix v of the output GGSW is the fp-ks
 * of w with key i.  ggsw_out is [num_samples][level_cbs][k+1][(k+1)N], level matrix 0 being decomposition
 * level 1 (the order concrete_hip_vertical_packing reads).  pbs_out: optional [num_samples][level_cbs][kN+1],
 * the rows w after the body constant (what the fp-ks reads).  Every pointer is device memory; fourier_bsk as
 * in concrete_hip_pbs.  scratch: 16-byte aligned, at least concrete_hip_circuit_bootstrap_scratch_bytes()
 * bytes, or NULL for stream-ordered pool scratch.  One batched PBS over num_samples * level_cbs rows, then one
 * fp-ks; stream-ordered, no host synchronisation, device-to-host copy or allocation in between.
 * Checked before the first device call: -1 null pointer; -3 delta_log > 63, sizes that overflow, a scratch
 * buffer too small or misaligned; -2 parameters for which concrete_hip_circuit_bootstrap_supported is 0 (also:
 * a key that fails the PBS exactness gate).  Nothing is written by a refused call. */
int concrete_hip_circuit_bootstrap(void *stream, uint32_t gpu_index, uint64_t *ggsw_out, const uint64_t *lwe_array_in,
                                   const void *fourier_bsk, const uint64_t *fp_ksk, uint32_t delta_log,
                                   uint32_t lwe_dimension, uint32_t glwe_dimension, uint32_t polynomial_size,
                                   uint32_t level_bsk, uint32_t base_log_bsk, uint32_t level_pksk,
                                   uint32_t base_log_pksk, uint32_t level_cbs, uint32_t base_log_cbs,
                                   uint32_t num_samples, void *scratch, uint64_t scratch_bytes, uint64_t *pbs_out);
/* scratch bytes of such a call; 0 for num_samples == 0, level_cbs == 0, lwe_dimension == 0, (k+1)N == 0 or
 * above 65536, or sizes that overflow.  Does not decrease with num_samples or level_cbs. */
uint64_t concrete_hip_circuit_bootstrap_scratch_bytes(uint32_t lwe_dimension, uint32_t glwe_dimension,
                                                      uint32_t polynomial_size, uint32_t level_cbs,
                                                      uint32_t num_samples);
/* 1 exactly when concrete_hip_pbs_supported(k, N, level_bsk, base_log_bsk), concrete_hip_keyswitch_supported(
 * level_pksk, base_log_pksk, kN + 1, (k+1)N - 1), level_cbs >= 1 and level_cbs * base_log_cbs <= 63 all hold */
int concrete_hip_circuit_bootstrap_supported(uint32_t glwe_dimension, uint32_t polynomial_size, uint32_t level_bsk,
                                             uint32_t base_log_bsk, uint32_t level_pksk, uint32_t base_log_pksk,
                                             uint32_t level_cbs, uint32_t base_log_cbs);
/* u64 words of the list of k + 1 fp-ks keys: (k+1) (kN+1) level (k+1)N; 0 when that overflows 64 bits */
uint64_t concrete_hip_fpksk_size_words(uint32_t glwe_dimension, uint32_t polynomial_size, uint32_t level_count);
/* The WoP-PBS end to end, with a status code.  One lookup with t boolean inputs and tau LUTs of
 * 2^t words: r = max(t - log2 N, 0), m = min(t, log2 N); concrete_hip_circuit_bootstrap over the t bit ciphertexts
 * at delta_log 63, whose output is the ggsw_in of concrete_hip_vertical_packing at (level_cbs, base_log_cbs), r,
 * mbr_size = m, tau.  The LUT operand [tau][2^r][N] is the cleartext array [tau][2^t] as it stands when
 * t >= log2 N (the caller's pointer is passed through); for t < log2 N the 2^t words go to the front of a zero
 * polynomial (concrete-cpu's Ordering::Less branch).
 * concrete_hip_circuit_bootstrap_vertical_packing: stages 2 and 3 for num_lookups lookups that share the LUTs.
 *   lwe_array_in   [num_lookups][number_of_inputs][lwe_dimension + 1], the bits at 2^63, most significant first
 *   lwe_array_out  [num_lookups][tau][kN+1]
 * concrete_hip_wop_pbs_crt: the CRT front of the runtime's memref_wop_pbs_crt_buffer (compiler lib/Runtime/
 * wrappers.cpp:903-965), stage 1, then the call above with num_lookups = batch.  Block i of modulus moduli[i]
 * (HOST array of num_blocks entries, each 2 .. 2^63) yields nb_i = ceil(log2 m_i) bits at delta_log 64 - nb_i
 * after 2^(63-nb_i) - 2^(59-nb_i) is taken off its body (the second term dropped when nb_i > 59); per value the
 * bits are ordered [block num_blocks-1 | ... | block 0], each most significant first; t = sum nb_i, tau =
 * num_blocks.  Stage 1 is a single concrete_hip_extract_bits over batch * num_blocks rows.
 *   lwe_array_in   [batch][num_blocks][kN+1], not modified
 *   cleartext_luts [num_blocks][2^t]
 *   lwe_array_out  [batch][num_blocks][kN+1]
 * Every other pointer is device memory too; fourier_bsk as in concrete_hip_pbs, ksk as in concrete_hip_keyswitch,
 * fp_ksk as in concrete_hip_circuit_bootstrap.  scratch: 16-byte aligned, at least
 * concrete_hip_wop_pbs_scratch_bytes() bytes, or NULL for stream-ordered pool scratch (one allocation); every
 * intermediate buffer is carved from it.  ggsw_spectrum_max: as concrete_hip_vertical_packing.  In the steady
 * state the whole call makes ONE host synchronisation of the stream, vertical packing's for its gate, and the
 * driver adds none.  What the stages may add, as in their own calls: the first PBS on a key that needs its
 * general-format companion builds it and synchronises once (concrete_hip_pbs), and bit extraction waits for the
 * calling thread's previous upload of index data, normally long done, before it reuses the staging block.
 * Checked before the first device call: -1 null pointer; -3 number_of_inputs == 0, tau == 0, num_blocks == 0 or
 * above 16, a modulus out of range, t > log2 N + 24, sizes that overflow, a scratch buffer too small or
 * misaligned; -2 parameters for which concrete_hip_wop_pbs_supported (for the first call: its last two
 * conditions) is 0.  A key or GGSWs that fail an exactness gate: -2.  A refused call leaves lwe_array_out
 * untouched. */
int concrete_hip_circuit_bootstrap_vertical_packing(
    void *stream, uint32_t gpu_index, uint64_t *lwe_array_out, const uint64_t *lwe_array_in,
    const uint64_t *cleartext_luts, const void *fourier_bsk, const uint64_t *fp_ksk, uint32_t lwe_dimension,
    uint32_t glwe_dimension, uint32_t polynomial_size, uint32_t level_bsk, uint32_t base_log_bsk, uint32_t level_pksk,
    uint32_t base_log_pksk, uint32_t level_cbs, uint32_t base_log_cbs, uint32_t number_of_inputs, uint32_t tau,
    uint32_t num_lookups, void *scratch, uint64_t scratch_bytes, double *ggsw_spectrum_max);
int concrete_hip_wop_pbs_crt(void *stream, uint32_t gpu_index, uint64_t *lwe_array_out, const uint64_t *lwe_array_in,
                             const uint64_t *cleartext_luts, const void *fourier_bsk, const uint64_t *ksk,
                             const uint64_t *fp_ksk, const uint64_t *moduli, uint32_t num_blocks, uint32_t batch,
                             uint32_t lwe_dimension, uint32_t glwe_dimension, uint32_t polynomial_size,
                             uint32_t level_bsk, uint32_t base_log_bsk, uint32_t level_ksk, uint32_t base_log_ksk,
                             uint32_t level_pksk, uint32_t base_log_pksk, uint32_t level_cbs, uint32_t base_log_cbs,
                             void *scratch, uint64_t scratch_bytes, double *ggsw_spectrum_max);
/* scratch bytes of a chained call on `batch` values (lookups) of number_of_bits = t boolean inputs and tau LUTs;
 * num_blocks: the stage-1 inputs per value (CRT blocks), 0 for concrete_hip_circuit_bootstrap_vertical_packing.
 * 0 for t == 0, tau == 0, batch == 0, level_cbs == 0, num_blocks > t, t > log2 N + 24, a shape a stage has no
 * scratch size for, or sizes that overflow.  Does not decrease with batch, t, tau or level_cbs. */
uint64_t concrete_hip_wop_pbs_scratch_bytes(uint32_t lwe_dimension, uint32_t glwe_dimension, uint32_t polynomial_size,
                                            uint32_t level_cbs, uint32_t num_blocks, uint32_t number_of_bits,
                                            uint32_t tau, uint32_t batch);
/* 1 exactly when concrete_hip_extract_bits_supported(kN, lwe_dimension, k, N, base_log_bsk, level_bsk, base_log_ksk,
 * level_ksk), concrete_hip_circuit_bootstrap_supported(k, N, level_bsk, base_log_bsk, level_pksk, base_log_pksk,
 * level_cbs, base_log_cbs) and concrete_hip_vertical_packing_supported(k, N, level_cbs, base_log_cbs) all hold */
int concrete_hip_wop_pbs_supported(uint32_t lwe_dimension, uint32_t glwe_dimension, uint32_t polynomial_size,
                                   uint32_t level_bsk, uint32_t base_log_bsk, uint32_t level_ksk, uint32_t base_log_ksk,
                                   uint32_t level_pksk, uint32_t base_log_pksk, uint32_t level_cbs,
                                   uint32_t base_log_cbs);
/* Fourier key registered for a `dest` of cuda_convert_lwe_programmable_bootstrap_key_64, or NULL */
const void *concrete_hip_lookup_bsk(const void *bootstrapping_key);
/* Release what the backend derived from device buffer `ptr` (a registered Fourier key whose `dest`
 * is ptr, the int8 key bytes the matrix-core keyswitch cached for a KSK at ptr — cached only for
 * buffers from cuda_malloc_async or a keyset) without freeing ptr itself; cuda_drop /
 * cuda_drop_async do this for every pointer, and cuda_memcpy_async_to_gpu for its destination.
 * Returns the number of cached key-byte entries released. */
int concrete_hip_release_device_buffer(const void *ptr);
/* LUT encoding on the device (compiler lib/Runtime/wrappers.cpp:388-450,
 * memref_encode_expand_lut_for_bootstrap, for num_luts rows at once): out is num_luts x out_size,
 * in is num_luts x in_size, device pointers; stream-ordered. */
int concrete_hip_encode_expand_lut_device(void *stream, uint32_t gpu_index, uint64_t *out, uint64_t out_size,
                                          const uint64_t *in, uint64_t in_size, uint64_t num_luts,
                                          uint32_t out_message_bits, int is_signed);
/* Trivial-GLWE accumulators on the device (wrappers.cpp:199-209): acc is num_luts x (k+1)N, row l =
 * k zero polynomials then LUT row l of luts (num_luts x N); device pointers; stream-ordered. */
int concrete_hip_build_accumulators(void *stream, uint32_t gpu_index, uint64_t *acc, const uint64_t *luts,
                                    uint64_t num_luts, uint32_t glwe_dim, uint32_t polynomial_size);
/* number of visible devices */
int concrete_hip_device_count(void);
/* Synchronise the device and return (and clear) the sticky status of every stream on it: 0 ok, -4
 * when a PBS kernel's wave synchronisation gave up after its spin bound since the last check (that
 * launch's outputs are wrong).  cuda_synchronize_device performs the same check and aborts. */
int concrete_hip_device_status(uint32_t gpu_index);
/* Stream-ordered status of one stream (round 5): waits for the work issued on `stream` (nothing
 * else), then returns (and clears) the status of the PBS launches made on that stream since its last
 * check: 0 ok, -4 when one of them gave up a wave synchronisation (its outputs are wrong).  Status
 * words are per (device, stream), so concurrent calls on other streams are never blamed. */
int concrete_hip_stream_status(void *stream, uint32_t gpu_index);
/* Spin bound (LDS-counter polls) of the PBS kernels' wave synchronisation for later launches;
 * 0 restores the default (2^22).  Test hook: a tiny bound forces the timeout path. */
void concrete_hip_set_spin_limit(uint32_t polls);
/* The same bound for launches issued by the calling host thread only (0: the process-wide bound).
 * Test hook: forces the timeout path on one of several concurrent calls. */
void concrete_hip_set_thread_spin_limit(uint32_t polls);
/* How a cfg2-shaped call (k = 1, N = 1024, l = 3) of num_samples ciphertexts is split on a device of
 * `cus` compute units (round 6): parts[0..2] = ciphertexts run on the pair kernel (4 per CU), the
 * six-wave kernel at 2 per CU and at 1 per CU, in that launch order; returns the estimated time in
 * 1/100 ms per round at n = 630 (concrete_amd/csrc/pbs1024_plan.hpp). */
uint64_t concrete_hip_pbs1024_plan(uint64_t num_samples, uint32_t cus, uint32_t *parts);
/* Status slots held by live streams of the device (round 6): a stream gets a slot on its first PBS
 * launch and returns it when it is destroyed (cuda_destroy_stream, the runtime's own streams), so a
 * caller that creates and destroys a stream per call (wrappers.cpp:129/160) never exhausts them. */
uint32_t concrete_hip_status_slots_in_use(uint32_t gpu_index);
/* Test hook: at most `slots` status slots per device (0 restores 4096); a stream arriving while all
 * are taken shares slot 0, whose reads still report that stream's launches. */
void concrete_hip_set_status_slot_cap(uint32_t slots);

/* ------------------------------------------------------------------------------------------
 * Part 3: client-side helpers (host code; synthetic workloads and LUT encoding).
 * INSECURE — FOR TESTS AND BENCHMARKS ONLY: keys, masks and noise come from xoshiro256** seeded
 * with the caller's 64-bit seed (Box-Muller Gaussians), not from a CSPRNG; reusing a seed reuses
 * the encryption masks.  Real key material comes from the reference's client (concrete-csprng).
 * Mirrors the
 * concrete-cpu client ABI (backends/concrete-cpu/implementation/include/concrete-cpu.h:
 * concrete_cpu_init_secret_key_u64, concrete_cpu_encrypt_lwe_ciphertext_u64,
 * concrete_cpu_init_lwe_bootstrap_key_u64, concrete_cpu_init_lwe_keyswitch_key_u64) and the
 * runtime's LUT expansion (compiler lib/Runtime/wrappers.cpp:388-450).  Deterministic per seed.
 * ------------------------------------------------------------------------------------------ */
double concrete_hip_secure_log2_std(uint64_t glwe_dim, uint64_t poly_size);
void concrete_hip_keygen_binary(uint64_t *sk, uint64_t len, uint64_t seed);
void concrete_hip_lwe_encrypt_batch(const uint64_t *sk, uint64_t *out, const uint64_t *plaintexts, uint64_t count,
                                    uint64_t n, double std_torus, uint64_t seed);
uint64_t concrete_hip_lwe_decrypt(const uint64_t *sk, const uint64_t *ct, uint64_t n);
void concrete_hip_bsk_generate(uint64_t *bsk, const uint64_t *lwe_sk, const uint64_t *glwe_sk, uint64_t n,
                               uint64_t k, uint64_t N, uint64_t l, uint64_t logB, double std_torus, uint64_t seed);
void concrete_hip_ksk_generate(uint64_t *ksk, const uint64_t *sk_in, const uint64_t *sk_out, uint64_t n_in,
                               uint64_t n_out, uint64_t l, uint64_t logB, double std_torus, uint64_t seed);
/* The list of k + 1 fp-ks keys of the circuit bootstrap (concrete_hip_fpksk_size_words(k, N, l) words, the
 * layout given with cuda_fp_keyswitch_lwe_to_glwe_64).  lwe_sk_in: the kN bits of the input LWE key, which is the
 * flattened GLWE key the PBS output is under; glwe_sk: the output GLWE key.  Entry (i, j, t) is a GLWE
 * encryption of -s_j 2^(64 - logB (l - t)) P_i, P_i = polynomial i of glwe_sk for i < k, P_k = the constant -1,
 * s_kN = -1.  Parallel over the (i, j) blocks, block b = i (kN + 1) + j seeded with
 * seed ^ (0x2545f491 * (b + 1)). */
void concrete_hip_fpksk_generate(uint64_t *fpksk, const uint64_t *lwe_sk_in, const uint64_t *glwe_sk, uint64_t k,
                                 uint64_t N, uint64_t l, uint64_t logB, double std_torus, uint64_t seed);
void concrete_hip_encode_expand_lut(uint64_t *out, uint64_t out_size, const uint64_t *in, uint64_t in_size,
                                    uint32_t out_message_bits, int is_signed);

/* ------------------------------------------------------------------------------------------
 * Part 4: circuit-facing runtime glue (SURVEY.md §8b layer B2).  Mirrors of the runtime's
 * memref wrappers (compiler include/concretelang/Runtime/wrappers.h:240-300, implementation
 * lib/Runtime/wrappers.cpp:88-363) over an opaque keyset handle instead of the C++
 * RuntimeContext (include/concretelang/Runtime/context.h:42-145): MLIR memref descriptors
 * expanded as (allocated, aligned, offset, sizes..., strides...), host memory in and out, the
 * same shape assertions (violations abort), trivial GLWE accumulators built from the LUT
 * (wrappers.cpp:199-209), one LUT per sample for the mapped form (wrappers.cpp:317-325).
 * Differences by design: device keys are converted once per keyset and device and reused
 * across calls (the reference re-converts per RuntimeContext, ServerLib.cpp:579); a keyset may
 * list several devices, across which every batched call is sharded in contiguous slices
 * (the reference's direct route is "TODO: Multi GPU", wrappers.cpp:176-177), the converted key
 * reaching the other devices by peer copy.
 * ------------------------------------------------------------------------------------------ */
typedef struct concrete_hip_keyset concrete_hip_keyset;
concrete_hip_keyset *concrete_hip_keyset_create(void);
void concrete_hip_keyset_destroy(concrete_hip_keyset *ks);
/* standard-domain keys (host buffers, copied): BSK [n][l][k+1][k+1][N], KSK [n_in][l][n_out+1] */
int concrete_hip_keyset_add_bsk(concrete_hip_keyset *ks, uint32_t bsk_index, const uint64_t *bsk, uint32_t input_lwe_dim,
                                uint32_t glwe_dim, uint32_t level, uint32_t base_log, uint32_t poly_size);
int concrete_hip_keyset_add_ksk(concrete_hip_keyset *ks, uint32_t ksk_index, const uint64_t *ksk, uint32_t level,
                                uint32_t base_log, uint32_t input_lwe_dim, uint32_t output_lwe_dim);
/* The list of k + 1 packing keyswitch (fp-ks) keys of a circuit bootstrap, under the index the runtime context
 * uses (context.h fp_keyswitch_key_buffer(pksk_index)): a host buffer of concrete_hip_fpksk_size_words(glwe_dim,
 * poly_size, level) words in the layout given with cuda_fp_keyswitch_lwe_to_glwe_64, copied; the key is uploaded
 * on first use, stays resident per device like a KSK, and is freed with the keyset.  input_lwe_dim must be
 * glwe_dim * poly_size.  -3 bad argument, -2 a (level, base_log) the fp-ks does not take. */
int concrete_hip_keyset_add_fpksk(concrete_hip_keyset *ks, uint32_t pksk_index, const uint64_t *fpksk, uint32_t level,
                                  uint32_t base_log, uint32_t input_lwe_dim, uint32_t glwe_dim, uint32_t poly_size);
/* devices the batched calls shard across (default: device 0); entries may repeat.  Every slice of
 * a call runs on its own host thread, stream and cached device buffers. */
int concrete_hip_keyset_set_devices(concrete_hip_keyset *ks, const uint32_t *devices, uint32_t count);
/* Diagnostics: record HIP events around every slice of the following calls ... */
void concrete_hip_keyset_set_timing(concrete_hip_keyset *ks, int enable);
/* ... and read them for every call since timing was enabled, in completion order: 6 doubles per
 * slice (device, then ms since timing was enabled on that device: slice start, inputs copied
 * (kernel issue), kernel done, outputs copied, then the slice's sample count); returns the number
 * of slices (copies at most max_slices).  Concurrent calls on one keyset run on slot sets of their
 * own, so their slices share this time axis (round 4). */
uint32_t concrete_hip_keyset_timeline(concrete_hip_keyset *ks, double *out, uint32_t max_slices);

/* The runtime's context pointer (mlir::concretelang::RuntimeContext *, context.h:42-154) is what
 * the circuit passes to memref_*_cuda_u64 and to the stream emulator's KS / PBS processes.  The
 * backend resolves it to a keyset: a pointer bound with concrete_hip_context_bind (NULL keyset
 * unbinds), else the resolver's answer (cached per context), else the pointer itself when it is a
 * live keyset handle.  An unresolvable context aborts (reference failure behaviour). */
int concrete_hip_context_bind(const void *runtime_context, concrete_hip_keyset *ks);
typedef concrete_hip_keyset *(*concrete_hip_context_resolver)(const void *runtime_context, void *user);
void concrete_hip_set_context_resolver(concrete_hip_context_resolver fn, void *user);

void memref_keyswitch_lwe_hip_u64(uint64_t *out_allocated, uint64_t *out_aligned, uint64_t out_offset,
                                  uint64_t out_size, uint64_t out_stride, uint64_t *ct0_allocated,
                                  uint64_t *ct0_aligned, uint64_t ct0_offset, uint64_t ct0_size, uint64_t ct0_stride,
                                  uint32_t level, uint32_t base_log, uint32_t input_lwe_dim,
                                  uint32_t output_lwe_dim, uint32_t ksk_index, concrete_hip_keyset *context);
void memref_bootstrap_lwe_hip_u64(uint64_t *out_allocated, uint64_t *out_aligned, uint64_t out_offset,
                                  uint64_t out_size, uint64_t out_stride, uint64_t *ct0_allocated,
                                  uint64_t *ct0_aligned, uint64_t ct0_offset, uint64_t ct0_size, uint64_t ct0_stride,
                                  uint64_t *tlu_allocated, uint64_t *tlu_aligned, uint64_t tlu_offset,
                                  uint64_t tlu_size, uint64_t tlu_stride, uint32_t input_lwe_dim, uint32_t poly_size,
                                  uint32_t level, uint32_t base_log, uint32_t glwe_dim, uint32_t bsk_index,
                                  concrete_hip_keyset *context);
void memref_batched_keyswitch_lwe_hip_u64(uint64_t *out_allocated, uint64_t *out_aligned, uint64_t out_offset,
                                          uint64_t out_size0, uint64_t out_size1, uint64_t out_stride0,
                                          uint64_t out_stride1, uint64_t *ct0_allocated, uint64_t *ct0_aligned,
                                          uint64_t ct0_offset, uint64_t ct0_size0, uint64_t ct0_size1,
                                          uint64_t ct0_stride0, uint64_t ct0_stride1, uint32_t level,
                                          uint32_t base_log, uint32_t input_lwe_dim, uint32_t output_lwe_dim,
                                          uint32_t ksk_index, concrete_hip_keyset *context);
void memref_batched_bootstrap_lwe_hip_u64(uint64_t *out_allocated, uint64_t *out_aligned, uint64_t out_offset,
                                          uint64_t out_size0, uint64_t out_size1, uint64_t out_stride0,
                                          uint64_t out_stride1, uint64_t *ct0_allocated, uint64_t *ct0_aligned,
                                          uint64_t ct0_offset, uint64_t ct0_size0, uint64_t ct0_size1,
                                          uint64_t ct0_stride0, uint64_t ct0_stride1, uint64_t *tlu_allocated,
                                          uint64_t *tlu_aligned, uint64_t tlu_offset, uint64_t tlu_size,
                                          uint64_t tlu_stride, uint32_t input_lwe_dim, uint32_t poly_size,
                                          uint32_t level, uint32_t base_log, uint32_t glwe_dim, uint32_t bsk_index,
                                          concrete_hip_keyset *context);
void memref_batched_mapped_bootstrap_lwe_hip_u64(
    uint64_t *out_allocated, uint64_t *out_aligned, uint64_t out_offset, uint64_t out_size0, uint64_t out_size1,
    uint64_t out_stride0, uint64_t out_stride1, uint64_t *ct0_allocated, uint64_t *ct0_aligned, uint64_t ct0_offset,
    uint64_t ct0_size0, uint64_t ct0_size1, uint64_t ct0_stride0, uint64_t ct0_stride1, uint64_t *tlu_allocated,
    uint64_t *tlu_aligned, uint64_t tlu_offset, uint64_t tlu_size0, uint64_t tlu_size1, uint64_t tlu_stride0,
    uint64_t tlu_stride1, uint32_t input_lwe_dim, uint32_t poly_size, uint32_t level, uint32_t base_log,
    uint32_t glwe_dim, uint32_t bsk_index, concrete_hip_keyset *context);
/* The CRT WoP-PBS of one value (compiler lib/Runtime/wrappers.cpp:855-997, memref_wop_pbs_crt_buffer: the same
 * argument list and shape assertions): out and in are (blocks, kN+1) host memrefs, lut_ct (blocks, 2^t) cleartext
 * LUTs with t = sum ceil(log2 m_i), crt_decomp the blocks' moduli.  One concrete_hip_wop_pbs_crt call with
 * batch = 1 on the keyset's first device (a WoP call is not sharded), with the keyset's resident BSK, KSK and
 * fp-ks keys, whose registered parameters must be the call's. */
void memref_wop_pbs_crt_buffer_hip_u64(
    uint64_t *out_allocated, uint64_t *out_aligned, uint64_t out_offset, uint64_t out_size_0, uint64_t out_size_1,
    uint64_t out_stride_0, uint64_t out_stride_1, uint64_t *in_allocated, uint64_t *in_aligned, uint64_t in_offset,
    uint64_t in_size_0, uint64_t in_size_1, uint64_t in_stride_0, uint64_t in_stride_1, uint64_t *lut_ct_allocated,
    uint64_t *lut_ct_aligned, uint64_t lut_ct_offset, uint64_t lut_ct_size0, uint64_t lut_ct_size1,
    uint64_t lut_ct_stride0, uint64_t lut_ct_stride1, uint64_t *crt_decomp_allocated, uint64_t *crt_decomp_aligned,
    uint64_t crt_decomp_offset, uint64_t crt_decomp_size, uint64_t crt_decomp_stride, uint32_t lwe_small_dim,
    uint32_t cbs_level_count, uint32_t cbs_base_log, uint32_t ksk_level_count, uint32_t ksk_base_log,
    uint32_t bsk_level_count, uint32_t bsk_base_log, uint32_t fpksk_level_count, uint32_t fpksk_base_log,
    uint32_t polynomial_size, uint32_t ksk_index, uint32_t bsk_index, uint32_t pksk_index,
    concrete_hip_keyset *context);

/* The direct GPU route under the reference's own names and argument lists
 * (compiler include/concretelang/Runtime/wrappers.h:246-300, lib/Runtime/wrappers.cpp:70-363):
 * `context` is the caller's runtime context, resolved as described above.  Same semantics as the
 * memref_*_hip_u64 forms (every batched call sharded over the keyset's devices). */
void memref_keyswitch_lwe_cuda_u64(uint64_t *out_allocated, uint64_t *out_aligned, uint64_t out_offset,
                                   uint64_t out_size, uint64_t out_stride, uint64_t *ct0_allocated,
                                   uint64_t *ct0_aligned, uint64_t ct0_offset, uint64_t ct0_size,
                                   uint64_t ct0_stride, uint32_t level, uint32_t base_log, uint32_t input_lwe_dim,
                                   uint32_t output_lwe_dim, uint32_t ksk_index, void *context);
void memref_bootstrap_lwe_cuda_u64(uint64_t *out_allocated, uint64_t *out_aligned, uint64_t out_offset,
                                   uint64_t out_size, uint64_t out_stride, uint64_t *ct0_allocated,
                                   uint64_t *ct0_aligned, uint64_t ct0_offset, uint64_t ct0_size,
                                   uint64_t ct0_stride, uint64_t *tlu_allocated, uint64_t *tlu_aligned,
                                   uint64_t tlu_offset, uint64_t tlu_size, uint64_t tlu_stride,
                                   uint32_t input_lwe_dim, uint32_t poly_size, uint32_t level, uint32_t base_log,
                                   uint32_t glwe_dim, uint32_t bsk_index, void *context);
void memref_batched_keyswitch_lwe_cuda_u64(uint64_t *out_allocated, uint64_t *out_aligned, uint64_t out_offset,
                                           uint64_t out_size0, uint64_t out_size1, uint64_t out_stride0,
                                           uint64_t out_stride1, uint64_t *ct0_allocated, uint64_t *ct0_aligned,
                                           uint64_t ct0_offset, uint64_t ct0_size0, uint64_t ct0_size1,
                                           uint64_t ct0_stride0, uint64_t ct0_stride1, uint32_t level,
                                           uint32_t base_log, uint32_t input_lwe_dim, uint32_t output_lwe_dim,
                                           uint32_t ksk_index, void *context);
void memref_batched_bootstrap_lwe_cuda_u64(uint64_t *out_allocated, uint64_t *out_aligned, uint64_t out_offset,
                                           uint64_t out_size0, uint64_t out_size1, uint64_t out_stride0,
                                           uint64_t out_stride1, uint64_t *ct0_allocated, uint64_t *ct0_aligned,
                                           uint64_t ct0_offset, uint64_t ct0_size0, uint64_t ct0_size1,
                                           uint64_t ct0_stride0, uint64_t ct0_stride1, uint64_t *tlu_allocated,
                                           uint64_t *tlu_aligned, uint64_t tlu_offset, uint64_t tlu_size,
                                           uint64_t tlu_stride, uint32_t input_lwe_dim, uint32_t poly_size,
                                           uint32_t level, uint32_t base_log, uint32_t glwe_dim, uint32_t bsk_index,
                                           void *context);
void memref_batched_mapped_bootstrap_lwe_cuda_u64(
    uint64_t *out_allocated, uint64_t *out_aligned, uint64_t out_offset, uint64_t out_size0, uint64_t out_size1,
    uint64_t out_stride0, uint64_t out_stride1, uint64_t *ct0_allocated, uint64_t *ct0_aligned, uint64_t ct0_offset,
    uint64_t ct0_size0, uint64_t ct0_size1, uint64_t ct0_stride0, uint64_t ct0_stride1, uint64_t *tlu_allocated,
    uint64_t *tlu_aligned, uint64_t tlu_offset, uint64_t tlu_size0, uint64_t tlu_size1, uint64_t tlu_stride0,
    uint64_t tlu_stride1, uint32_t input_lwe_dim, uint32_t poly_size, uint32_t level, uint32_t base_log,
    uint32_t glwe_dim, uint32_t bsk_index, void *context);
/* memref_wop_pbs_crt_buffer with the context resolved as above.  The reference has no GPU variant of this
 * wrapper: the compiler's CAPI lowering has to emit this name for the op. */
void memref_wop_pbs_crt_buffer_cuda_u64(
    uint64_t *out_allocated, uint64_t *out_aligned, uint64_t out_offset, uint64_t out_size_0, uint64_t out_size_1,
    uint64_t out_stride_0, uint64_t out_stride_1, uint64_t *in_allocated, uint64_t *in_aligned, uint64_t in_offset,
    uint64_t in_size_0, uint64_t in_size_1, uint64_t in_stride_0, uint64_t in_stride_1, uint64_t *lut_ct_allocated,
    uint64_t *lut_ct_aligned, uint64_t lut_ct_offset, uint64_t lut_ct_size0, uint64_t lut_ct_size1,
    uint64_t lut_ct_stride0, uint64_t lut_ct_stride1, uint64_t *crt_decomp_allocated, uint64_t *crt_decomp_aligned,
    uint64_t crt_decomp_offset, uint64_t crt_decomp_size, uint64_t crt_decomp_stride, uint32_t lwe_small_dim,
    uint32_t cbs_level_count, uint32_t cbs_base_log, uint32_t ksk_level_count, uint32_t ksk_base_log,
    uint32_t bsk_level_count, uint32_t bsk_base_log, uint32_t fpksk_level_count, uint32_t fpksk_base_log,
    uint32_t polynomial_size, uint32_t ksk_index, uint32_t bsk_index, uint32_t pksk_index, void *context);

/* ------------------------------------------------------------------------------------------
 * Part 5: the SDFG stream emulator — the default GPU route of a circuit compiled with SDFG
 * extraction (compiler include/concretelang/Runtime/stream_emulator_api.h:30-106; reference
 * implementation lib/Runtime/GPUDFG.cpp:1467-1799; call sequence emitted by
 * lib/Conversion/SDFGToStreamEmulator/SDFGToStreamEmulator.cpp:25-73: init, make streams, make
 * processes, run, put inputs, get outputs, delete).  Same names and argument lists; `stype` is the
 * reference's `stream_type` enum (passed as int; values below).  A get evaluates the processes its
 * stream depends on whose inputs changed since their last evaluation, the whole subgraph resident
 * on the devices (sdfg.hip).  Devices: CONCRETE_HIP_SDFG_DEVICES ("0,0,1", repeats allowed), else
 * SDFG_NUM_GPUS, else all visible devices.  `context` of KS / PBS processes: as in Part 4.
 * ------------------------------------------------------------------------------------------ */
enum {
  CONCRETE_HIP_TS_STREAM_TYPE_X86_TO_TOPO_LSAP = 0,
  CONCRETE_HIP_TS_STREAM_TYPE_TOPO_TO_TOPO_LSAP = 1,
  CONCRETE_HIP_TS_STREAM_TYPE_TOPO_TO_X86_LSAP = 2,
  CONCRETE_HIP_TS_STREAM_TYPE_TOPO_TO_BOTH = 3,
  CONCRETE_HIP_TS_STREAM_TYPE_X86_TO_X86_LSAP = 4
};
void *stream_emulator_init(void);
void stream_emulator_run(void *dfg);
void stream_emulator_delete(void *dfg);
void stream_emulator_make_memref_add_lwe_ciphertexts_u64_process(void *dfg, void *sin1, void *sin2, void *sout);
void stream_emulator_make_memref_add_plaintext_lwe_ciphertext_u64_process(void *dfg, void *sin1, void *sin2,
                                                                          void *sout);
void stream_emulator_make_memref_mul_cleartext_lwe_ciphertext_u64_process(void *dfg, void *sin1, void *sin2,
                                                                          void *sout);
void stream_emulator_make_memref_negate_lwe_ciphertext_u64_process(void *dfg, void *sin1, void *sout);
void stream_emulator_make_memref_keyswitch_lwe_u64_process(void *dfg, void *sin1, void *sout, uint32_t level,
                                                           uint32_t base_log, uint32_t input_lwe_dim,
                                                           uint32_t output_lwe_dim, uint32_t output_size,
                                                           uint32_t ksk_index, void *context);
void stream_emulator_make_memref_bootstrap_lwe_u64_process(void *dfg, void *sin1, void *sin2, void *sout,
                                                           uint32_t input_lwe_dim, uint32_t poly_size,
                                                           uint32_t level, uint32_t base_log, uint32_t glwe_dim,
                                                           uint32_t output_size, uint32_t bsk_index, void *context);
void stream_emulator_make_memref_batched_add_lwe_ciphertexts_u64_process(void *dfg, void *sin1, void *sin2,
                                                                         void *sout);
void stream_emulator_make_memref_batched_add_plaintext_lwe_ciphertext_u64_process(void *dfg, void *sin1, void *sin2,
                                                                                  void *sout);
void stream_emulator_make_memref_batched_add_plaintext_cst_lwe_ciphertext_u64_process(void *dfg, void *sin1,
                                                                                      void *sin2, void *sout);
void stream_emulator_make_memref_batched_mul_cleartext_lwe_ciphertext_u64_process(void *dfg, void *sin1, void *sin2,
                                                                                  void *sout);
void stream_emulator_make_memref_batched_mul_cleartext_cst_lwe_ciphertext_u64_process(void *dfg, void *sin1,
                                                                                      void *sin2, void *sout);
void stream_emulator_make_memref_batched_negate_lwe_ciphertext_u64_process(void *dfg, void *sin1, void *sout);
void stream_emulator_make_memref_batched_keyswitch_lwe_u64_process(void *dfg, void *sin1, void *sout, uint32_t level,
                                                                   uint32_t base_log, uint32_t input_lwe_dim,
                                                                   uint32_t output_lwe_dim, uint32_t output_size,
                                                                   uint32_t ksk_index, void *context);
void stream_emulator_make_memref_batched_bootstrap_lwe_u64_process(void *dfg, void *sin1, void *sin2, void *sout,
                                                                   uint32_t input_lwe_dim, uint32_t poly_size,
                                                                   uint32_t level, uint32_t base_log,
                                                                   uint32_t glwe_dim, uint32_t output_size,
                                                                   uint32_t bsk_index, void *context);
void stream_emulator_make_memref_batched_mapped_bootstrap_lwe_u64_process(void *dfg, void *sin1, void *sin2,
                                                                          void *sout, uint32_t input_lwe_dim,
                                                                          uint32_t poly_size, uint32_t level,
                                                                          uint32_t base_log, uint32_t glwe_dim,
                                                                          uint32_t output_size, uint32_t bsk_index,
                                                                          void *context);
void *stream_emulator_make_uint64_stream(const char *name, int stype);
void stream_emulator_put_uint64(void *stream, uint64_t e);
uint64_t stream_emulator_get_uint64(void *stream);
void *stream_emulator_make_memref_stream(const char *name, int stype);
void stream_emulator_put_memref(void *stream, uint64_t *allocated, uint64_t *aligned, uint64_t offset, uint64_t size,
                                uint64_t stride, uint64_t data_ownership);
void stream_emulator_get_memref(void *stream, uint64_t *out_allocated, uint64_t *out_aligned, uint64_t out_offset,
                                uint64_t out_size, uint64_t out_stride);
void *stream_emulator_make_memref_batch_stream(const char *name, int stype);
void stream_emulator_put_memref_batch(void *stream, uint64_t *allocated, uint64_t *aligned, uint64_t offset,
                                      uint64_t size0, uint64_t size1, uint64_t stride0, uint64_t stride1,
                                      uint64_t data_ownership);
void stream_emulator_get_memref_batch(void *stream, uint64_t *out_allocated, uint64_t *out_aligned,
                                      uint64_t out_offset, uint64_t out_size0, uint64_t out_size1,
                                      uint64_t out_stride0, uint64_t out_stride1);

/* ------------------------------------------------------------------------------------------
 * Part 6: key wire-format import (concrete_amd/csrc/keyio.cpp).
 * Reads the evaluation keys of a serialized concrete keyset — the Cap'n Proto messages
 * `ServerKeyset.serialize()` / `Keyset.serialize()` write (capnp::writeMessage, unpacked framing,
 * include/concretelang/Common/Protocol.h:158-175; schema tools/concrete-protocol/src/
 * concrete-protocol.capnp:149-297) — and registers them in a runtime keyset under the indexes the
 * runtime context uses (list position, lib/Runtime/context.cpp:36-94), replacing the reference's
 * ServerKeyset::fromProto + LweBootstrapKey/LweKeyswitchKey::fromProto (lib/Common/Keys.cpp:142-163,
 * 262-283).  Payloads: List(Data) blobs concatenated (Protocol.h:349-372).  Seeded keys
 * (Compression::SEED, Keys.cpp:193-218) are expanded by concrete-cpu's own decompressors, which the
 * caller installs (the runtime already links concrete-cpu); without them a seeded key is refused.
 * Only 64-bit keys over the native modulus are accepted (the PBS / KS kernels' torus).
 * Returns 0, or < 0 with concrete_hip_last_error() set (malformed message, size mismatch, ...).
 * ------------------------------------------------------------------------------------------ */
typedef struct concrete_hip_server_keyset concrete_hip_server_keyset;
enum {
  CONCRETE_HIP_ROOT_SERVER_KEYSET = 0,    /* ServerKeyset (ServerKeyset.serialize()) */
  CONCRETE_HIP_ROOT_KEYSET = 1,           /* Keyset: its `server` part (Keyset.serialize()) */
  CONCRETE_HIP_ROOT_LWE_BOOTSTRAP_KEY = 2, /* one LweBootstrapKey */
  CONCRETE_HIP_ROOT_LWE_KEYSWITCH_KEY = 3  /* one LweKeyswitchKey */
};
typedef struct concrete_hip_key_info {
  uint32_t id, input_id, output_id;          /* LweBootstrapKeyInfo / LweKeyswitchKeyInfo */
  uint32_t level_count, base_log;
  uint32_t glwe_dim, poly_size;              /* bootstrap keys only */
  uint32_t input_lwe_dim, output_lwe_dim;    /* bootstrap keys: output = glwe_dim * poly_size */
  uint32_t integer_precision;
  uint32_t key_type;                         /* KeyType: 0 binary, 1 ternary */
  uint32_t compression;                      /* Compression: 0 none, 1 seed, 2 paillier */
  uint32_t modulus_kind, modulus_value;      /* Modulus union: 0 native, 1 power of two, 2 integer */
  double variance;
  uint64_t payload_words;                    /* u64 words on the wire */
  uint64_t key_words;                        /* u64 words of the standard-domain key */
} concrete_hip_key_info;
int concrete_hip_server_keyset_deserialize(const void *bytes, uint64_t size, uint32_t root,
                                           concrete_hip_server_keyset **out);
int concrete_hip_server_keyset_load_file(const char *path, uint32_t root, concrete_hip_server_keyset **out);
void concrete_hip_server_keyset_destroy(concrete_hip_server_keyset *sk);
uint32_t concrete_hip_server_keyset_bsk_count(const concrete_hip_server_keyset *sk);
uint32_t concrete_hip_server_keyset_ksk_count(const concrete_hip_server_keyset *sk);
int concrete_hip_server_keyset_bsk_info(const concrete_hip_server_keyset *sk, uint32_t index,
                                        concrete_hip_key_info *out);
int concrete_hip_server_keyset_ksk_info(const concrete_hip_server_keyset *sk, uint32_t index,
                                        concrete_hip_key_info *out);
/* the standard-domain key (BSK [n][l][k+1][k+1][N], KSK [n_in][l][n_out+1]); dst holds >= key_words */
/* Level order of evaluation key `index` (is_bsk: bootstrap, else keyswitch), found when it was last
 * read (read_bsk / read_ksk / keyset_add_server_keyset) against the client secret keys a Keyset
 * message carries: one GGSW / keyswitch row per level is decrypted.  A key stored in the reversed
 * level order is re-ordered on read; one that decrypts in neither order is refused (round 4). */
enum {
  CONCRETE_HIP_LEVEL_ORDER_UNCHECKED = 0,   /* no client keys (ServerKeyset), one level, or not read yet */
  CONCRETE_HIP_LEVEL_ORDER_AS_EXPECTED = 1, /* the order the standard layouts assume */
  CONCRETE_HIP_LEVEL_ORDER_REVERSED = 2     /* stored reversed: re-ordered on read */
};
int concrete_hip_server_keyset_level_order(const concrete_hip_server_keyset *sk, int is_bsk, uint32_t index);
/* client secret keys read from a Keyset message (0 for the other roots) */
uint32_t concrete_hip_server_keyset_secret_count(const concrete_hip_server_keyset *sk);
int concrete_hip_server_keyset_read_bsk(const concrete_hip_server_keyset *sk, uint32_t index, uint64_t *dst,
                                        uint64_t dst_words);
int concrete_hip_server_keyset_read_ksk(const concrete_hip_server_keyset *sk, uint32_t index, uint64_t *dst,
                                        uint64_t dst_words);
/* every bootstrap key i -> bsk_index i, every keyswitch key i -> ksk_index i */
int concrete_hip_keyset_add_server_keyset(concrete_hip_keyset *ks, const concrete_hip_server_keyset *sk);
/* Same layout and calling convention as concrete-cpu's Uint128 and its decompressors
 * (backends/concrete-cpu/implementation/include/concrete-cpu.h:49-51,185-207), so
 * concrete_cpu_decompress_seeded_lwe_{bootstrap,keyswitch}_key_u64 install directly.  The last
 * argument is concrete-cpu's Parallelism (1 = Rayon, what Keys.cpp:209-211 passes). */
typedef struct concrete_hip_uint128 {
  uint8_t little_endian_bytes[16];
} concrete_hip_uint128;
typedef void (*concrete_hip_bsk_decompressor)(uint64_t *lwe_bsk, const uint64_t *seeded_lwe_bsk,
                                              size_t input_lwe_dimension, size_t output_polynomial_size,
                                              size_t output_glwe_dimension, size_t decomposition_level_count,
                                              size_t decomposition_base_log, concrete_hip_uint128 compression_seed,
                                              uint32_t parallelism);
typedef void (*concrete_hip_ksk_decompressor)(uint64_t *lwe_ksk, const uint64_t *seeded_lwe_ksk,
                                              size_t input_lwe_dimension, size_t output_lwe_dimension,
                                              size_t decomposition_level_count, size_t decomposition_base_log,
                                              concrete_hip_uint128 compression_seed, uint32_t parallelism);
void concrete_hip_set_seeded_key_decompressors(concrete_hip_bsk_decompressor bsk, concrete_hip_ksk_decompressor ksk);

#ifdef __cplusplus
}
#endif
#endif /* CONCRETE_HIP_H */
