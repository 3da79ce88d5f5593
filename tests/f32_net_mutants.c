/* f32_net_mutants.c -- wrong twins of tests/f32_net_ref.c, each ONE change of the true chain, built the same way
 * (gcc -std=c11 -O2 -ffp-contract=off).  tests/test_f32_edges_ref.py shows that the operands the GPU tests of the f32
 * kernels use (tests/test_gpu_f32_exact.py) tell every one of them from the true chain; nothing else calls this file.
 * With mut = MUT_NONE every function below computes what f32_net_ref.c computes (asserted there too). */
#include <math.h>
#include <stddef.h>

enum {
  MUT_NONE = 0,
  MUT_NATURAL = 1,       /* (a) k in natural order inside a block of 16 */
  MUT_DROP_LAST = 2,     /* (b) the last block of 16 dropped */
  MUT_BIAS_START = 3,    /* (c) the chain started at bias instead of +0.0f, no add afterwards */
  MUT_RELU_FIRST = 4,    /* (d) ReLU before the bias add */
  MUT_NEXT_ROW = 5,      /* (e) row m reads row m + 1 (the last row itself) */
  MUT_NO_EDGE = 6,       /* (f) conv: a tap read without the board-edge test: the flat cell-major neighbour */
  MUT_NO_RESIDUAL = 7,   /* (g) conv: y = relu(s) */
  MUT_SWAP_PLANES = 8,   /* (h) conv0: the two input planes swapped */
  MUT_VALUE_ROW0 = 9     /* (i) head: value weights row 1 read as row 0 (f32mut_linear with n_cols == 2) */
};

static float chain(const float* w, const float* x, int k_len, float start, int mut) {
  float acc = start;
  if (mut == MUT_DROP_LAST) k_len -= 16;
  for (int kb = 0; kb < k_len; kb += 16) {
    if (mut == MUT_NATURAL) {
      for (int i = 0; i < 16; i++) acc = fmaf(w[kb + i], x[kb + i], acc);
    } else {
      for (int j = 0; j < 4; j++)
        for (int h = 0; h < 4; h++) acc = fmaf(w[kb + 4 * h + j], x[kb + 4 * h + j], acc);
    }
  }
  return acc;
}

static float relu(float s) { return s > 0.f ? s : 0.f; }

/* s of the true chain, or of the mutants that change how the bias joins it */
static float pre(const float* w, const float* x, int k_len, float b, int act, int mut) {
  if (mut == MUT_BIAS_START) return chain(w, x, k_len, b, mut);
  const float c = chain(w, x, k_len, 0.0f, mut);
  if (mut == MUT_RELU_FIRST && act) return relu(c) + b;
  return c + b;
}

void f32mut_linear(const float* x, int ldx, const float* w, const float* b, float* y, int ldy, int n_rows, int n_cols, int k_len, int act,
                   int mut) {
  for (int m = 0; m < n_rows; m++)
    for (int n = 0; n < n_cols; n++) {
      const int mr = mut == MUT_NEXT_ROW && m + 1 < n_rows ? m + 1 : m;
      const int nr = mut == MUT_VALUE_ROW0 && n_cols == 2 ? 0 : n;
      const float s = pre(w + (size_t)nr * k_len, x + (size_t)mr * ldx, k_len, b[n], act, mut);
      y[(size_t)m * ldy + n] = act && mut != MUT_RELU_FIRST ? relu(s) : s;
    }
}

void f32mut_conv0(const float* planes, int n_boards, int cp, const float* w0, const float* b, float* y, int mut) {
  float col[32];
  for (int g = 0; g < n_boards; g++)
    for (int cell = 0; cell < 42; cell++) {
      const int row = cell / 7, c = cell % 7;
      for (int k = 0; k < 32; k++) {
        const int tap = k >> 1, ci = mut == MUT_SWAP_PLANES ? 1 - (k & 1) : (k & 1), rr = row + tap / 3 - 1, cc = c + tap % 3 - 1;
        col[k] = (k < 18 && rr >= 0 && rr < 6 && cc >= 0 && cc < 7) ? planes[(size_t)g * 84 + ci * 42 + rr * 7 + cc] : 0.0f;
      }
      for (int n = 0; n < cp; n++) y[((size_t)g * 42 + cell) * cp + n] = pre(w0 + (size_t)n * 32, col, 32, b[n], 0, mut);
    }
}

void f32mut_conv(const float* x, int n_boards, int cp, const float* w, const float* b, float* y, const float* resid, int mut) {
  float col[9 * 64];
  for (int g = 0; g < n_boards; g++)
    for (int cell = 0; cell < 42; cell++) {
      const int row = cell / 7, c = cell % 7;
      for (int tap = 0; tap < 9; tap++) {
        const int rr = row + tap / 3 - 1, cc = c + tap % 3 - 1;
        int in = rr >= 0 && rr < 6 && cc >= 0 && cc < 7;
        if (mut == MUT_NO_EDGE) {   /* the flat neighbour: the next row or the next board (zero only outside the whole array) */
          const long flat = (long)g * 42 + rr * 7 + cc;
          in = flat >= 0 && flat < (long)n_boards * 42;
        }
        for (int ci = 0; ci < cp; ci++) col[tap * cp + ci] = in ? x[((long)g * 42 + rr * 7 + cc) * cp + ci] : 0.0f;
      }
      for (int n = 0; n < cp; n++) {
        const size_t o = ((size_t)g * 42 + cell) * cp + n;
        /* the residual convolution's ReLU is its activation: (d) moves it before the bias add there too */
        const float s = pre(w + (size_t)n * 9 * cp, col, 9 * cp, b[n], resid != NULL, mut);
        const float r = mut == MUT_RELU_FIRST ? s : relu(s);
        y[o] = resid ? (mut == MUT_NO_RESIDUAL ? r : resid[o] + r) : s;
      }
    }
}
