/* The vertical-packing declarations of include/concrete_hip.h from C99: the device-free queries, and every
 * refusal concrete_hip_vertical_packing makes before its first device call (tests/test_vertical_packing_abi.py
 * runs this with no visible device, where a device call would abort the process). */
#include <stdio.h>
#include <string.h>

#include "concrete_hip.h"

/* k = 1, N = 1024, l = 3 / logB = 8; a tree of 3 bits, a rotation of 4, 3 outputs, 2 lookups */
enum { K = 1, N = 1024, BL = 8, LV = 3, R = 3, MBR = 4, TAU = 3, LOOKUPS = 2 };

static uint64_t dummy[4]; /* stands for device memory: a refused call never reads it */
static int failures = 0;

static void expect(const char *what, int rc, int want) {
  const char *msg = concrete_hip_last_error();
  if (rc != want || msg == NULL || strstr(msg, "vertical_packing") == NULL) {
    printf("FAIL %s: rc %d (want %d), message \"%s\"\n", what, rc, want, msg ? msg : "(null)");
    ++failures;
  }
}

static int call(uint64_t *lwe, uint64_t *tree, const uint64_t *ggsw, const uint64_t *lut, uint32_t k, uint32_t n,
                uint32_t bl, uint32_t lv, uint32_t r, uint32_t mbr, uint32_t tau, uint32_t lookups, void *scratch,
                uint64_t scratch_bytes) {
  return concrete_hip_vertical_packing(NULL, 0, lwe, tree, ggsw, lut, k, n, bl, lv, r, mbr, tau, lookups, scratch,
                                       scratch_bytes, NULL, NULL);
}

int main(void) {
  static uint64_t small_scratch[4];
  static char raw[64];
  void *misaligned = (void *)((((uintptr_t)raw + 15) & ~(uintptr_t)15) + 8);
  /* function pointers: the reference's names are declared with the reference's argument lists */
  void (*tree_fn)(void *, uint32_t, void *, const void *, const void *, int8_t *, uint32_t, uint32_t, uint32_t, uint32_t,
                  uint32_t, uint32_t, uint32_t) = cuda_cmux_tree_64;
  void (*rot_fn)(void *, uint32_t, void *, const void *, const void *, int8_t *, uint32_t, uint32_t, uint32_t, uint32_t,
                 uint32_t, uint32_t, uint32_t) = cuda_blind_rotate_and_sample_extraction_64;
  void (*s1)(void *, uint32_t, int8_t **, uint32_t, uint32_t, uint32_t, uint32_t, uint32_t, uint32_t, bool) =
      scratch_cuda_cmux_tree_64;
  void (*s2)(void *, uint32_t, int8_t **, uint32_t, uint32_t, uint32_t, uint32_t, uint32_t, uint32_t, bool) =
      scratch_cuda_blind_rotation_sample_extraction_64;
  void (*c1)(void *, uint32_t, int8_t **) = cleanup_cuda_cmux_tree;
  void (*c2)(void *, uint32_t, int8_t **) = cleanup_cuda_blind_rotation_sample_extraction;
  int8_t *buf = (int8_t *)dummy;
  if (!tree_fn || !rot_fn || !s1 || !s2 || !c1 || !c2) ++failures;

  if (concrete_hip_abi_version() != 5) {
    printf("FAIL abi version %u\n", concrete_hip_abi_version());
    ++failures;
  }
  if (concrete_hip_vertical_packing_supported(K, N, LV, BL) != 1 ||
      concrete_hip_vertical_packing_supported(K, 1000, LV, BL) != 0 ||
      concrete_hip_vertical_packing_supported(K, N, LV, 40) != 0) {
    printf("FAIL supported\n");
    ++failures;
  }
  if (concrete_hip_vertical_packing_scratch_bytes(K, N, LV, R, MBR, TAU, LOOKUPS) == 0 ||
      concrete_hip_vertical_packing_scratch_bytes(K, N, LV, 25, MBR, TAU, LOOKUPS) != 0 ||
      concrete_hip_vertical_packing_scratch_bytes(K, N, LV, R, 11, TAU, LOOKUPS) != 0 ||
      concrete_hip_vertical_packing_scratch_bytes(K, N, LV, R, MBR, 0, LOOKUPS) != 0) {
    printf("FAIL scratch bytes\n");
    ++failures;
  }
  /* without allocation the scratch calls leave NULL and touch no device; cleanup of NULL is a no-op */
  s1(NULL, 0, &buf, K, N, LV, R, TAU, 0, false);
  if (buf != NULL) ++failures;
  c1(NULL, 0, &buf);
  buf = (int8_t *)dummy;
  s2(NULL, 0, &buf, K, N, LV, MBR, TAU, 0, false);
  if (buf != NULL) ++failures;
  c2(NULL, 0, &buf);

  expect("null LUTs", call(dummy, dummy, dummy, NULL, K, N, BL, LV, R, MBR, TAU, LOOKUPS, NULL, 0), -1);
  expect("null GGSWs", call(dummy, dummy, NULL, dummy, K, N, BL, LV, R, MBR, TAU, LOOKUPS, NULL, 0), -1);
  expect("tau == 0", call(dummy, dummy, dummy, dummy, K, N, BL, LV, R, MBR, 0, LOOKUPS, NULL, 0), -3);
  expect("num_lookups == 0", call(dummy, dummy, dummy, dummy, K, N, BL, LV, R, MBR, TAU, 0, NULL, 0), -3);
  expect("mbr_size > log2 N", call(dummy, dummy, dummy, dummy, K, N, BL, LV, R, 11, TAU, LOOKUPS, NULL, 0), -3);
  expect("r > 24", call(dummy, dummy, dummy, dummy, K, N, BL, LV, 25, MBR, TAU, LOOKUPS, NULL, 0), -3);
  expect("sizes overflow", call(dummy, dummy, dummy, dummy, K, N, BL, LV, 24, MBR, 0xffffffffu, 0xffffffffu, NULL, 0),
         -3);
  expect("no LWE output with a rotation", call(NULL, dummy, dummy, dummy, K, N, BL, LV, R, MBR, TAU, LOOKUPS, NULL, 0),
         -3);
  expect("no output at all", call(NULL, NULL, dummy, dummy, K, N, BL, LV, R, 0, TAU, LOOKUPS, NULL, 0), -3);
  expect("unsupported digits", call(dummy, dummy, dummy, dummy, K, N, 40, LV, R, MBR, TAU, LOOKUPS, NULL, 0), -2);
  expect("unsupported polynomial size", call(dummy, dummy, dummy, dummy, K, 4096, BL, LV, R, MBR, TAU, LOOKUPS, NULL, 0),
         -2);
  expect("unsupported GLWE dimension", call(dummy, dummy, dummy, dummy, 4, 512, BL, LV, R, MBR, TAU, LOOKUPS, NULL, 0),
         -2);
  expect("scratch too small",
         call(dummy, dummy, dummy, dummy, K, N, BL, LV, R, MBR, TAU, LOOKUPS, small_scratch, sizeof small_scratch), -3);
  expect("scratch misaligned",
         call(dummy, dummy, dummy, dummy, K, N, BL, LV, R, MBR, TAU, LOOKUPS, misaligned, 1ull << 40),
         -3);

  if (failures) return 1;
  printf("vertical_packing_client ok\n");
  return 0;
}
