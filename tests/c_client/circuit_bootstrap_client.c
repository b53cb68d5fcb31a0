/* The circuit-bootstrap declarations of include/concrete_hip.h from C99: the device-free queries, and every
 * refusal concrete_hip_circuit_bootstrap and concrete_hip_fp_keyswitch make before their first device call
 * (tests/test_circuit_bootstrap_abi.py runs this with no visible device, where a device call would abort the
 * process). */
#include <stdio.h>
#include <string.h>

#include "concrete_hip.h"

/* a row of the optimizer's WoP table: k = 2, N = 1024, br (3, 12), pp (2, 17), cb (2, 8); n = 620 */
enum { LWE_N = 620, K = 2, N = 1024, BL = 3, BB = 12, PL = 2, PB = 17, CL = 2, CB = 8, ROWS = 3 };

static uint64_t dummy[4]; /* stands for device memory: a refused call never reads it */
static int failures = 0;

static void expect(const char *what, const char *who, int rc, int want) {
  const char *msg = concrete_hip_last_error();
  if (rc != want || (want != 0 && (msg == NULL || strstr(msg, who) == NULL))) {
    printf("FAIL %s: rc %d (want %d), message \"%s\"\n", what, rc, want, msg ? msg : "(null)");
    ++failures;
  }
}

static int cbs(const void *in, uint32_t delta_log, uint32_t n_poly, uint32_t bl, uint32_t bb, uint32_t pl, uint32_t pb,
               uint32_t cl, uint32_t cb, uint32_t rows, void *scratch, uint64_t scratch_bytes) {
  return concrete_hip_circuit_bootstrap(NULL, 0, dummy, (const uint64_t *)in, dummy, dummy, delta_log, LWE_N, K, n_poly,
                                        bl, bb, pl, pb, cl, cb, rows, scratch, scratch_bytes, NULL);
}

static int fpks(const void *in, uint32_t n_in, uint32_t level, uint32_t base_log, uint32_t rows, uint32_t keys) {
  return concrete_hip_fp_keyswitch(NULL, 0, dummy, (const uint64_t *)in, dummy, n_in, K, N, base_log, level, rows,
                                   keys);
}

int main(void) {
  static uint64_t small_scratch[4];
  const char *c = "circuit_bootstrap", *f = "fp_keyswitch";

  if (concrete_hip_abi_version() != 5) {
    printf("FAIL abi version %u\n", concrete_hip_abi_version());
    ++failures;
  }
  if (concrete_hip_circuit_bootstrap_supported(K, N, BL, BB, PL, PB, CL, CB) != 1 ||
      concrete_hip_circuit_bootstrap_supported(K, N, BL, BB, PL, PB, 0, CB) != 0 ||
      concrete_hip_circuit_bootstrap_supported(K, N, BL, BB, PL, PB, 8, CB) != 0 ||
      concrete_hip_circuit_bootstrap_supported(K, N, BL, BB, 4, 16, CL, CB) != 0) {
    printf("FAIL supported\n");
    ++failures;
  }
  if (concrete_hip_circuit_bootstrap_scratch_bytes(LWE_N, K, N, CL, ROWS) == 0 ||
      concrete_hip_circuit_bootstrap_scratch_bytes(LWE_N, K, N, CL, 0) != 0 ||
      concrete_hip_circuit_bootstrap_scratch_bytes(LWE_N, K, N, 0, ROWS) != 0) {
    printf("FAIL scratch bytes\n");
    ++failures;
  }
  if (concrete_hip_fpksk_size_words(K, N, PL) != 3ull * 2049 * 2 * 3072) {
    printf("FAIL fpksk words\n");
    ++failures;
  }

  expect("cbs: no rows", c, cbs(dummy, 63, N, BL, BB, PL, PB, CL, CB, 0, NULL, 0), 0);
  expect("cbs: null input", c, cbs(NULL, 63, N, BL, BB, PL, PB, CL, CB, ROWS, NULL, 0), -1);
  expect("cbs: delta_log > 63", c, cbs(dummy, 64, N, BL, BB, PL, PB, CL, CB, ROWS, NULL, 0), -3);
  expect("cbs: unsupported PBS digits", c, cbs(dummy, 63, N, 3, 40, PL, PB, CL, CB, ROWS, NULL, 0), -2);
  expect("cbs: unsupported polynomial size", c, cbs(dummy, 63, 1000, BL, BB, PL, PB, CL, CB, ROWS, NULL, 0), -2);
  expect("cbs: unsupported fp-ks digits", c, cbs(dummy, 63, N, BL, BB, 4, 16, CL, CB, ROWS, NULL, 0), -2);
  expect("cbs: no cbs level", c, cbs(dummy, 63, N, BL, BB, PL, PB, 0, CB, ROWS, NULL, 0), -2);
  expect("cbs: cbs digits past 63 bits", c, cbs(dummy, 63, N, BL, BB, PL, PB, 8, CB, ROWS, NULL, 0), -2);
  expect("cbs: sizes overflow", c, cbs(dummy, 63, N, BL, BB, PL, PB, CL, CB, 0xffffffffu, NULL, 0), -3);
  expect("cbs: scratch too small", c,
         cbs(dummy, 63, N, BL, BB, PL, PB, CL, CB, ROWS, small_scratch, sizeof small_scratch), -3);

  expect("fpks: no rows", f, fpks(dummy, K * N, PL, PB, 0, K + 1), 0);
  expect("fpks: null input", f, fpks(NULL, K * N, PL, PB, ROWS, K + 1), -1);
  expect("fpks: no keys", f, fpks(dummy, K * N, PL, PB, ROWS, 0), -3);
  expect("fpks: n_in != k N", f, fpks(dummy, K * N + 1, PL, PB, ROWS, K + 1), -3);
  expect("fpks: sizes overflow", f, fpks(dummy, K * N, PL, PB, 0xffffffffu, K + 1), -3);
  expect("fpks: unsupported digits", f, fpks(dummy, K * N, 4, 16, ROWS, K + 1), -2);

  if (failures) return 1;
  printf("circuit_bootstrap_client ok\n");
  return 0;
}
