// sg_lstm.hip -- the recurrence of one direction of one fp64 LSTM layer with H = 128 hidden units (include/softgrip.h: sg_lstm_forward,
// sg_lstm_backward; soft-grip_amd/lstm.py is the caller).  What is regular stays with the caller's GEMMs -- the input projection
// z = x.kernel + bias for all time steps, and the weight gradients over the stored sequences -- and these two kernels do what is serial
// in time: one persistent launch per call that walks all T steps with h and c on chip.
//
// Layout, both kernels.  A workgroup of 4 wavefronts owns BT = 16 batch rows for all T steps; the grid is ceil(B / 16) -- at B = 4096 one
// workgroup on each of the 256 CUs.  Wavefront w owns the hidden units 32w .. 32w+31 in all four gates, as two column tiles (j = 0, 1) of
// v_mfma_f64_16x16x4_f64.  That instruction's result map is NOT the other MFMAs': lane l holds column l & 15 and, in result register r,
// row (l >> 4) + 4r; its operands are one f64 per lane, A[row l & 15][k l >> 4] and B[k l >> 4][column l & 15].  With the batch rows as
// the tile's rows and the units as its columns, lane l therefore holds, for r = 0..3 and j = 0, 1, the element
//     (row (l >> 4) + 4r, unit 32w + 16j + (l & 15))
// of every gate: the cell update is register-local, and c (forward) and dc (backward) never leave registers.
//
// U is read as the caller holds it, row-major [H][4H], straight from L2 every step (512 KB: neither LDS nor registers hold it) with no
// re-packing and no scratch: in the forward product a 16-lane group reads 16 consecutive doubles of one row of U -- one whole 128-byte
// line -- and in the backward product, which needs U transposed, a lane reads 4 consecutive k of its own row of U (32 bytes) and the
// four lane groups of a column complete the line; the MFMA's k index is then a permutation of memory order, which a sum over k does not
// mind as long as the A operand (from LDS) follows the same permutation.
//
// No atomics, no reductions across workgroups: two runs give the same bits, and a batch row's result does not depend on B.
#include <hip/hip_runtime.h>

#include <string>

#include "../../include/softgrip.h"
#include "sg_batch.h"   // fail, HIPCHK

namespace {

constexpr int LH = 128, LG = 4 * LH, LBT = 16;
typedef double lstm_d4 __attribute__((ext_vector_type(4)));

__device__ inline double lstm_sigmoid(double x) { return 1.0 / (1.0 + exp(-x)); }

// forward.  LDS: h of the previous and of this step, each [k = unit][row] (16 KB): lane l's A operand of k-step ks is word 64 ks + l.
__global__ __launch_bounds__(256) void sg_lstm_fwd_kernel(int B, int T, double* __restrict__ z, const double* __restrict__ U,
                                                          const double* __restrict__ h0, const double* __restrict__ c0,
                                                          double* __restrict__ h_seq, double* __restrict__ h_last,
                                                          double* __restrict__ c_last, double* __restrict__ c_seq, int save) {
  __shared__ double hs[2][LH * LBT];
  const int lane = threadIdx.x & 63, w = threadIdx.x >> 6, l15 = lane & 15, q = lane >> 4;
  const long long b0 = (long long)blockIdx.x * LBT;
  const int u0 = 32 * w + l15;          // this lane's unit for j = 0; + 16 for j = 1

  double c[2][4];
#pragma unroll
  for (int j = 0; j < 2; j++)
#pragma unroll
    for (int r = 0; r < 4; r++) {
      const int row = q + 4 * r, u = u0 + 16 * j;
      const long long b = b0 + row;
      const bool ok = b < B;
      c[j][r] = (c0 && ok) ? c0[b * LH + u] : 0.0;
      hs[0][u * LBT + row] = (h0 && ok) ? h0[b * LH + u] : 0.0;
    }

  // the pre-activations of step t, fetched one step ahead: they are the accumulators' initial value
  lstm_d4 zn[4][2];
  auto load_z = [&](int t) {
#pragma unroll
    for (int g = 0; g < 4; g++)
#pragma unroll
      for (int j = 0; j < 2; j++)
#pragma unroll
        for (int r = 0; r < 4; r++) {
          const long long b = b0 + q + 4 * r;
          zn[g][j][r] = b < B ? z[((size_t)b * T + t) * LG + g * LH + u0 + 16 * j] : 0.0;
        }
  };
  load_z(0);

  // U's fragments, fetched one group of LKG k-steps ahead of the MFMAs that use them, in two register sets (a group's 32 MFMAs are
  // 2048 cycles, about what a load from L2 takes); the first group of the NEXT time step is fetched before this step's cell update
  // and barrier, which it does not depend on
  constexpr int LKG = 4;
  const double* Uw = U + (size_t)q * LG + u0;
  double ua[LKG][8], ub[LKG][8];
  auto load_u = [&](double (&u)[LKG][8], int kg) {
#pragma unroll
    for (int kk = 0; kk < LKG; kk++)
#pragma unroll
      for (int g = 0; g < 4; g++)
#pragma unroll
        for (int j = 0; j < 2; j++) u[kk][2 * g + j] = Uw[(size_t)(kg * LKG + kk) * 4 * LG + g * LH + 16 * j];    // U[4 ks + q][...]
  };
  load_u(ua, 0);
  __syncthreads();

  for (int t = 0; t < T; t++) {
    const int cur = t & 1;
    lstm_d4 acc[4][2];
#pragma unroll
    for (int g = 0; g < 4; g++)
#pragma unroll
      for (int j = 0; j < 2; j++) acc[g][j] = zn[g][j];
    if (t + 1 < T) load_z(t + 1);

    const double* hb = hs[cur];
    auto mac = [&](const double (&u)[LKG][8], int kg) {
#pragma unroll
      for (int kk = 0; kk < LKG; kk++) {
        const double a = hb[(kg * LKG + kk) * 64 + lane];    // h[row l15][k = 4 ks + q]
#pragma unroll
        for (int g = 0; g < 4; g++)
#pragma unroll
          for (int j = 0; j < 2; j++) acc[g][j] = __builtin_amdgcn_mfma_f64_16x16x4f64(a, u[kk][2 * g + j], acc[g][j], 0, 0, 0);
      }
    };
#pragma unroll 1
    for (int kg = 0; kg < LH / 4 / LKG; kg += 2) {
      load_u(ub, kg + 1);
      mac(ua, kg);
      load_u(ua, kg + 2 < LH / 4 / LKG ? kg + 2 : 0);       // (past the last group: the next step's first; unused after step T - 1)
      mac(ub, kg + 1);
    }

    double* hn = hs[cur ^ 1];
#pragma unroll
    for (int j = 0; j < 2; j++)
#pragma unroll
      for (int r = 0; r < 4; r++) {
        const int row = q + 4 * r, u = u0 + 16 * j;
        const long long b = b0 + row;
        const double gi = lstm_sigmoid(acc[0][j][r]), gf = lstm_sigmoid(acc[1][j][r]), gg = tanh(acc[2][j][r]), go = lstm_sigmoid(acc[3][j][r]);
        const double cn = gf * c[j][r] + gi * gg;
        const double h = go * tanh(cn);
        c[j][r] = cn;
        hn[u * LBT + row] = h;
        if (b < B) {                                       // rows past B: computed on zeros, never written
          const size_t bt = (size_t)b * T + t;
          if (save) {
            double* zo = z + bt * LG + u;
            zo[0] = gi, zo[LH] = gf, zo[2 * LH] = gg, zo[3 * LH] = go;
            c_seq[bt * LH + u] = cn;
          }
          if (h_seq) h_seq[bt * LH + u] = h;
          if (t == T - 1) {
            if (h_last) h_last[b * LH + u] = h;
            if (c_last) c_last[b * LH + u] = cn;
          }
        }
      }
    __syncthreads();     // h of this step is whole before the next step's product reads it; nobody still reads the other buffer
  }
}

// what the backward pointwise stage of one step reads for a lane's 8 elements, fetched one step ahead
struct LstmBwdIn {
  double gi[2][4], gf[2][4], gg[2][4], go[2][4], ct[2][4], cp[2][4], dh[2][4];
};

// backward.  LDS: the dz tile of this step (64 KB) in the order the product's A operand is read: element (row, k) at word
// (((k >> 4) * 4 + (k & 3)) * 4 + ((k >> 2) & 3)) * 16 + row, so that lane l's operand of k-step (kb, s) is word 64 (4 kb + s) + l.
__global__ __launch_bounds__(256) void sg_lstm_bwd_kernel(int B, int T, const double* __restrict__ gates, const double* __restrict__ c_seq,
                                                          const double* __restrict__ c0, const double* __restrict__ U,
                                                          const double* __restrict__ dh_seq, const double* __restrict__ dh_last,
                                                          double* __restrict__ dz, double* __restrict__ dh0, double* __restrict__ dc0) {
  __shared__ double ds[LBT * LG];
  const int lane = threadIdx.x & 63, w = threadIdx.x >> 6, l15 = lane & 15, q = lane >> 4;
  const long long b0 = (long long)blockIdx.x * LBT;
  const int u0 = 32 * w + l15;

  LstmBwdIn nx;
  auto load_in = [&](int t) {
#pragma unroll
    for (int j = 0; j < 2; j++)
#pragma unroll
      for (int r = 0; r < 4; r++) {
        const int u = u0 + 16 * j;
        const long long b = b0 + q + 4 * r;
        const bool ok = b < B;
        const size_t bt = ok ? (size_t)b * T + t : 0;
        const double* gp = gates + bt * LG + u;
        nx.gi[j][r] = ok ? gp[0] : 0.0;
        nx.gf[j][r] = ok ? gp[LH] : 0.0;
        nx.gg[j][r] = ok ? gp[2 * LH] : 0.0;
        nx.go[j][r] = ok ? gp[3 * LH] : 0.0;
        nx.ct[j][r] = ok ? c_seq[bt * LH + u] : 0.0;
        nx.cp[j][r] = !ok ? 0.0 : t > 0 ? c_seq[(bt - 1) * LH + u] : c0 ? c0[b * LH + u] : 0.0;
        double d = (ok && dh_seq) ? dh_seq[bt * LH + u] : 0.0;
        if (ok && dh_last && t == T - 1) d += dh_last[b * LH + u];
        nx.dh[j][r] = d;
      }
  };
  load_in(T - 1);

  double dc[2][4];
  lstm_d4 rec[2];
#pragma unroll
  for (int j = 0; j < 2; j++)
#pragma unroll
    for (int r = 0; r < 4; r++) dc[j][r] = 0.0, rec[j][r] = 0.0;

  // U's fragments one group of LKG blocks of 16 k ahead, as in the forward kernel: U[n][16 kb + 4 q + s] for the lane's two units
  constexpr int LKG = 4;
  const double* Un = U + (size_t)u0 * LG + 4 * q;
  double ua[LKG][8], ub[LKG][8];
  auto load_u = [&](double (&u)[LKG][8], int kg) {
#pragma unroll
    for (int kk = 0; kk < LKG; kk++)
#pragma unroll
      for (int j = 0; j < 2; j++)
#pragma unroll
        for (int s = 0; s < 4; s++) u[kk][4 * j + s] = Un[(size_t)16 * j * LG + 16 * (kg * LKG + kk) + s];
  };
  load_u(ua, 0);

  for (int t = T - 1; t >= 0; t--) {
    const LstmBwdIn in = nx;
    if (t > 0) load_in(t - 1);
#pragma unroll
    for (int j = 0; j < 2; j++)
#pragma unroll
      for (int r = 0; r < 4; r++) {
        const int row = q + 4 * r, u = u0 + 16 * j;
        const long long b = b0 + row;
        const double gi = in.gi[j][r], gf = in.gf[j][r], gg = in.gg[j][r], go = in.go[j][r];
        const double dh = in.dh[j][r] + rec[j][r];
        const double tc = tanh(in.ct[j][r]);
        const double dcv = dc[j][r] + dh * go * (1.0 - tc * tc);
        dc[j][r] = dcv * gf;
        double zz[4];
        zz[0] = dcv * gg * gi * (1.0 - gi);
        zz[1] = dcv * in.cp[j][r] * gf * (1.0 - gf);
        zz[2] = dcv * gi * (1.0 - gg * gg);
        zz[3] = dh * tc * go * (1.0 - go);
#pragma unroll
        for (int g = 0; g < 4; g++) {
          const int k = g * LH + u;
          ds[(((k >> 4) * 4 + (k & 3)) * 4 + ((k >> 2) & 3)) * 16 + row] = zz[g];   // (rows past B: zeros in, zeros out)
        }
        if (b < B) {
          double* zo = dz + ((size_t)b * T + t) * LG + u;
          zo[0] = zz[0], zo[LH] = zz[1], zo[2 * LH] = zz[2], zo[3 * LH] = zz[3];
        }
      }
    __syncthreads();

    // dh_rec[row][n] = sum_k dz[row][k] U[n][k], n = this wavefront's 32 units; two accumulators per tile keep the MFMA pipe fed
    lstm_d4 acc[2][2];
#pragma unroll
    for (int j = 0; j < 2; j++)
#pragma unroll
      for (int e = 0; e < 2; e++)
#pragma unroll
        for (int r = 0; r < 4; r++) acc[j][e][r] = 0.0;
    auto mac = [&](const double (&u)[LKG][8], int kg) {
#pragma unroll
      for (int kk = 0; kk < LKG; kk++)
#pragma unroll
        for (int s = 0; s < 4; s++) {
          const double a = ds[((kg * LKG + kk) * 4 + s) * 64 + lane];                      // dz[row l15][16 kb + 4 q + s]
#pragma unroll
          for (int j = 0; j < 2; j++) acc[j][s & 1] = __builtin_amdgcn_mfma_f64_16x16x4f64(a, u[kk][4 * j + s], acc[j][s & 1], 0, 0, 0);
        }
    };
#pragma unroll 1
    for (int kg = 0; kg < LG / 16 / LKG; kg += 2) {
      load_u(ub, kg + 1);
      mac(ua, kg);
      load_u(ua, kg + 2 < LG / 16 / LKG ? kg + 2 : 0);      // (past the last group: the next step's first)
      mac(ub, kg + 1);
    }
#pragma unroll
    for (int j = 0; j < 2; j++) rec[j] = acc[j][0] + acc[j][1];
    __syncthreads();     // the product has read the tile before the next step overwrites it
  }

#pragma unroll
  for (int j = 0; j < 2; j++)
#pragma unroll
    for (int r = 0; r < 4; r++) {
      const int u = u0 + 16 * j;
      const long long b = b0 + q + 4 * r;
      if (b < B) {
        if (dh0) dh0[b * LH + u] = rec[j][r];
        if (dc0) dc0[b * LH + u] = dc[j][r];
      }
    }
}

}  // namespace

extern "C" {

int sg_lstm_forward(int B, int T, int H, double* z, const double* U, const double* h0, const double* c0, double* h_seq, double* h_last,
                    double* c_last, double* c_seq, int save, void* stream) {
  if (B <= 0 || T <= 0) return fail(SG_ERR_INVALID, "sg_lstm_forward: B and T must be positive");
  if (H != LH) return fail(SG_ERR_INVALID, "sg_lstm_forward: H must be 128, got " + std::to_string(H));
  if (!z || !U) return fail(SG_ERR_INVALID, "sg_lstm_forward: null z or U");
  if (save && !c_seq) return fail(SG_ERR_INVALID, "sg_lstm_forward: save needs c_seq");
  hipLaunchKernelGGL(sg_lstm_fwd_kernel, dim3((unsigned)((B + LBT - 1) / LBT)), dim3(256), 0, (hipStream_t)stream, B, T, z, U, h0, c0, h_seq,
                     h_last, c_last, c_seq, save);
  HIPCHK(hipGetLastError());
  return SG_OK;
}

int sg_lstm_backward(int B, int T, int H, const double* gates, const double* c_seq, const double* c0, const double* U, const double* dh_seq,
                     const double* dh_last, double* dz, double* dh0, double* dc0, void* stream) {
  if (B <= 0 || T <= 0) return fail(SG_ERR_INVALID, "sg_lstm_backward: B and T must be positive");
  if (H != LH) return fail(SG_ERR_INVALID, "sg_lstm_backward: H must be 128, got " + std::to_string(H));
  if (!gates || !c_seq || !U || !dz) return fail(SG_ERR_INVALID, "sg_lstm_backward: null gates, c_seq, U or dz");
  hipLaunchKernelGGL(sg_lstm_bwd_kernel, dim3((unsigned)((B + LBT - 1) / LBT)), dim3(256), 0, (hipStream_t)stream, B, T, gates, c_seq, c0, U,
                     dh_seq, dh_last, dz, dh0, dc0);
  HIPCHK(hipGetLastError());
  return SG_OK;
}

}  // extern "C"
