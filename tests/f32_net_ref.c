/* f32_net_ref.c -- plain-C restatement of the f32 evaluator's summation order (include/c4a0_hip.h, "f32 evaluator"), the
 * oracle the hand-written f32 kernels (c4a0_amd/csrc/c4_f32_net.hip) are compared with bit for bit.  Built with
 * -ffp-contract=off: every product-and-add below is the explicit fmaf, every other operation a separately rounded f32 op.
 * Weights come in the layouts of c4a0_amd.nn.pack_f32_weights. */
#include <math.h>
#include <stddef.h>

/* the documented chain: +0.0f, then k = kb + 4 h + j for blocks kb of 16, j = 0..3 (outer), h = 0..3 */
static float chain(const float* w, const float* x, int k_len) {
  float acc = 0.0f;
  for (int kb = 0; kb < k_len; kb += 16)
    for (int j = 0; j < 4; j++)
      for (int h = 0; h < 4; h++) acc = fmaf(w[kb + 4 * h + j], x[kb + 4 * h + j], acc);
  return acc;
}

static float relu(float s) { return s > 0.f ? s : 0.f; }

/* y[m][n] = act(chain(w[n], x[m]) + b[n]); act 0 = none, 1 = relu */
void f32ref_linear(const float* x, int ldx, const float* w, const float* b, float* y, int ldy, int n_rows, int n_cols, int k_len, int act) {
  for (int m = 0; m < n_rows; m++)
    for (int n = 0; n < n_cols; n++) {
      const float s = chain(w + (size_t)n * k_len, x + (size_t)m * ldx, k_len) + b[n];
      y[(size_t)m * ldy + n] = act ? relu(s) : s;
    }
}

/* conv0: planes [G][2][6][7] -> y [G][42][cp]; w0 [cp][32], k = 2 tap + ci (< 18) */
void f32ref_conv0(const float* planes, int n_boards, int cp, const float* w0, const float* b, float* y) {
  float col[32];
  for (int g = 0; g < n_boards; g++)
    for (int cell = 0; cell < 42; cell++) {
      const int row = cell / 7, c = cell % 7;
      for (int k = 0; k < 32; k++) {
        const int tap = k >> 1, ci = k & 1, rr = row + tap / 3 - 1, cc = c + tap % 3 - 1;
        col[k] = (k < 18 && rr >= 0 && rr < 6 && cc >= 0 && cc < 7) ? planes[(size_t)g * 84 + ci * 42 + rr * 7 + cc] : 0.0f;
      }
      for (int n = 0; n < cp; n++) y[((size_t)g * 42 + cell) * cp + n] = chain(w0 + (size_t)n * 32, col, 32) + b[n];
    }
}

/* conv: x [G][42][cp] -> y [G][42][cp]; w [cp][9 cp], k = tap cp + ci.  resid NULL: y = s; else y = resid + relu(s)
 * (resid may be y itself: each element is read before it is written) */
void f32ref_conv(const float* x, int n_boards, int cp, const float* w, const float* b, float* y, const float* resid) {
  float col[9 * 64];
  for (int g = 0; g < n_boards; g++)
    for (int cell = 0; cell < 42; cell++) {
      const int row = cell / 7, c = cell % 7;
      for (int tap = 0; tap < 9; tap++) {
        const int rr = row + tap / 3 - 1, cc = c + tap % 3 - 1;
        const int in = rr >= 0 && rr < 6 && cc >= 0 && cc < 7;
        for (int ci = 0; ci < cp; ci++) col[tap * cp + ci] = in ? x[((size_t)g * 42 + rr * 7 + cc) * cp + ci] : 0.0f;
      }
      for (int n = 0; n < cp; n++) {
        const size_t o = ((size_t)g * 42 + cell) * cp + n;
        const float s = chain(w + (size_t)n * 9 * cp, col, 9 * cp) + b[n];
        y[o] = resid ? resid[o] + relu(s) : s;
      }
    }
}
