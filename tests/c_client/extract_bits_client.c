/* The bit-extraction declarations of include/concrete_hip.h from C99: the device-free queries, and every
 * refusal concrete_hip_extract_bits makes before its first device call (tests/test_extract_bits_abi.py runs
 * this with no visible device, where a device call would abort the process). */
#include <stdio.h>
#include <string.h>

#include "concrete_hip.h"

/* cfg2's shape: kN = 1024 -> n = 630, PBS l = 3 / logB = 7, KS l = 4 / logB = 3 */
enum { N_IN = 1024, N_OUT = 630, K = 1, N = 1024, BL = 7, LV = 3, KBL = 3, KLV = 4, ROWS = 3 };

static uint64_t dummy[4]; /* stands for device memory: a refused call never reads it */
static int failures = 0;

static void expect(const char *what, int rc, int want) {
  const char *msg = concrete_hip_last_error();
  if (rc != want || (want != 0 && (msg == NULL || strstr(msg, "extract_bits") == NULL))) {
    printf("FAIL %s: rc %d (want %d), message \"%s\"\n", what, rc, want, msg ? msg : "(null)");
    ++failures;
  }
}

static int call(const uint32_t *nb, const uint32_t *dl, const uint64_t *offs, uint32_t n_in, uint32_t n, uint32_t bl,
                uint32_t lv, uint32_t kbl, uint32_t klv, uint32_t rows, void *scratch, uint64_t scratch_bytes) {
  return concrete_hip_extract_bits(NULL, 0, dummy, dummy, dummy, dummy, nb, dl, offs, n_in, N_OUT, K, n, bl, lv, kbl,
                                   klv, rows, scratch, scratch_bytes);
}

int main(void) {
  const uint32_t nb[ROWS] = {2, 3, 1}, dl[ROWS] = {62, 61, 63};
  const uint32_t nb_zero[ROWS] = {2, 0, 1}, dl_zero[ROWS] = {62, 0, 63}, dl_wide[ROWS] = {62, 62, 63};
  const uint64_t perm[ROWS] = {4, 1, 0}, overlap[ROWS] = {0, 1, 5}, outside[ROWS] = {0, 2, 6};
  static uint64_t small_scratch[4];

  if (concrete_hip_abi_version() != 5) {
    printf("FAIL abi version %u\n", concrete_hip_abi_version());
    ++failures;
  }
  if (concrete_hip_extract_bits_supported(N_IN, N_OUT, K, N, BL, LV, KBL, KLV) != 1 ||
      concrete_hip_extract_bits_supported(N_IN + 1, N_OUT, K, N, BL, LV, KBL, KLV) != 0) {
    printf("FAIL supported\n");
    ++failures;
  }
  if (concrete_hip_extract_bits_scratch_bytes(N_IN, N_OUT, K, N, ROWS, 3) == 0) {
    printf("FAIL scratch bytes\n");
    ++failures;
  }

  expect("no rows", call(nb, dl, NULL, N_IN, N, BL, LV, KBL, KLV, 0, NULL, 0), 0);
  expect("null arrays", call(NULL, dl, NULL, N_IN, N, BL, LV, KBL, KLV, ROWS, NULL, 0), -1);
  expect("nb == 0", call(nb_zero, dl, NULL, N_IN, N, BL, LV, KBL, KLV, ROWS, NULL, 0), -3);
  expect("dl == 0", call(nb, dl_zero, NULL, N_IN, N, BL, LV, KBL, KLV, ROWS, NULL, 0), -3);
  expect("dl + nb > 64", call(nb, dl_wide, NULL, N_IN, N, BL, LV, KBL, KLV, ROWS, NULL, 0), -3);
  expect("n_in != k N", call(nb, dl, NULL, N_IN + 1, N, BL, LV, KBL, KLV, ROWS, NULL, 0), -3);
  expect("overlapping blocks", call(nb, dl, overlap, N_IN, N, BL, LV, KBL, KLV, ROWS, NULL, 0), -3);
  expect("block outside the output", call(nb, dl, outside, N_IN, N, BL, LV, KBL, KLV, ROWS, NULL, 0), -3);
  expect("unsupported PBS digits", call(nb, dl, perm, N_IN, N, 40, 3, KBL, KLV, ROWS, NULL, 0), -2);
  expect("unsupported polynomial size", call(nb, dl, perm, 1000, 1000, BL, LV, KBL, KLV, ROWS, NULL, 0), -2);
  expect("unsupported keyswitch", call(nb, dl, perm, N_IN, N, BL, LV, 16, 4, ROWS, NULL, 0), -2);
  expect("scratch too small", call(nb, dl, perm, N_IN, N, BL, LV, KBL, KLV, ROWS, small_scratch, sizeof small_scratch),
         -3);

  if (failures) return 1;
  printf("extract_bits_client ok\n");
  return 0;
}
