// kernels_wavecls.hpp -- gfx950 device code of the class form of the zonal-wavenumber fit
// (pytemdiags_amd/include_wavecls/temx_wavecls.h; the host side of its tables is wave_class_tables.hpp).
//
// Columns of one class side share Pbar_l^m(sin lat) and their row Z_s of P Ym (P the plan's native zonal-mean
// operator; a row of P Ym is a function of latitude alone), so
//     (Ym - P Ym)^T x = sum_sides Pbar(lat_s) (x) [sum_i x_i cos(m lon_i), sum_i x_i sin(m lon_i)] - Z_s sum_i x_i.
// The sweep is project_cls_kernel<T, 4, 1, ..> of kernels_cls.hpp with three sums per side instead of one: per member
// row three fused multiply-adds, per class-group and accumulator block three MFMAs -- the class basis against
// (Sc_N +- Sc_S) or (Ss_N +- Ss_S), and the deflation tables -E, -O (Z_N = E + O, Z_S = E - O) against S0_N + S0_S and
// S0_N - S0_S.  One field per wave, the plan's row table and work cuts (not group-aligned: partial sums are projected
// at the end of a piece), X loads and weight pairs PD - 1 batches ahead with the indices one batch further, the group's
// table staged in wave-private LDS, no workgroup barrier.  Everything is summed in fp64 whatever T is.
#pragma once
#include "kernels_cls.hpp"
#include "kernels_wave.hpp"
#include "wave_class_tables.hpp"

namespace temx {

// Class basis blocks of every class-group: one thread per class (ncls_pad = 4 (groups + 1); classes >= ncls are zero).
// tab is zeroed by the caller: the slots of degree offsets >= ndeg stay zero.
__global__ void __launch_bounds__(256)
wavecls_basis_kernel(const double* __restrict__ xc, int64_t ncls, int64_t ncls_pad, int m, int L, double pmm_norm, int TBS,
                     double* __restrict__ tab) {
  const int64_t ci = blockIdx.x * (int64_t)blockDim.x + threadIdx.x;
  if (ci >= ncls) return;
  double* blk = tab + (ci >> 2) * (int64_t)wavecls_group_doubles(TBS);
  const int k = (int)(ci & 3);
  wave_pbar_each(m, L, xc[ci], pmm_norm, [&](int r, double p) { blk[wavecls_basis_slot(TBS, r, k)] = p; });
}

// Deflation blocks: -E and -O of every class from the rows of Z = P Ym [N][Kc] at the class's representatives
// (rep[2 ci + side], -1: a side without members, whose sums are zero: Z_S := 0).  One thread per (class, column).
__global__ void __launch_bounds__(256)
wavecls_defl_kernel(const double* __restrict__ Z, const int* __restrict__ rep, int64_t ncls, int ndeg, int TBS,
                    double* __restrict__ tab) {
  const int Kc = 2 * ndeg;
  const int64_t idx = blockIdx.x * (int64_t)blockDim.x + threadIdx.x;
  if (idx >= ncls * Kc) return;
  const int64_t ci = idx / Kc;
  const int j = (int)(idx - ci * Kc), k = (int)(ci & 3);
  const int rn = rep[2 * ci], rs = rep[2 * ci + 1];
  const double zn = rn >= 0 ? Z[(int64_t)rn * Kc + j] : 0.0, zs = rs >= 0 ? Z[(int64_t)rs * Kc + j] : 0.0;
  double* blk = tab + (ci >> 2) * (int64_t)wavecls_group_doubles(TBS);
  blk[wavecls_defl_slot(TBS, ndeg, j, k, 0)] = -0.5 * (zn + zs);
  blk[wavecls_defl_slot(TBS, ndeg, j, k, 1)] = -0.5 * (zn - zs);
}

// partial[split][f][j][d] = (Ym - P Ym)^T x_f over this piece's member rows, j < Kc = 2 ndeg.
// NF = 4: the four waves of a workgroup are the four fields of a d-tile; NF = 1: four d-tiles of the one field.
template <typename T, int NF, int TBS, int WPS, int PD>
__global__ void __launch_bounds__(256, WPS)
wavecls_project_kernel(FieldPtrs<NF> fp, int64_t D, int ndeg, const double* __restrict__ tab,
                       const int4* __restrict__ crow, const double2* __restrict__ cw, const int2* __restrict__ csplit,
                       const double* __restrict__ colscale, int sfield, double* __restrict__ partial, int nsplit, int ndt) {
  static_assert(NF == 1 || NF == 4, "one field per wave: four fields or four d-tiles per workgroup");
  constexpr int DPW = 4 / NF;
  constexpr int NB = 2 * TBS, NA = 4 * TBS;
  constexpr int YE = wavecls_basis_doubles(TBS), ZE = wavecls_defl_doubles(TBS), TE = wavecls_group_doubles(TBS);
  constexpr int TJ = (TE + 63) / 64;
  constexpr int MB = CLS_MB;
  __shared__ double stage[4][TE];             // wave private
  int split, dq;
  if (!wg_work((ndt + DPW - 1) / DPW, nsplit, split, dq)) return;
  const int wave = uniform_wave(), lane = threadIdx.x & 63;
  const int c = lane & 15, g = lane >> 4;
  const int dt = dq * DPW + wave % DPW;
  const int f0 = wave / DPW;
  if (dt >= ndt) return;                      // (no barriers below)
  const int64_t d = (int64_t)dt * 16 + c;
  const bool dvalid = d < D;
  const int64_t dcl = dvalid ? d : D - 1;
  const int b0 = __builtin_amdgcn_readfirstlane(csplit[split].x);
  const int b1 = __builtin_amdgcn_readfirstlane(csplit[split + 1].x);
  int grp = __builtin_amdgcn_readfirstlane(csplit[split].y);
  const uint32_t yoff = (uint32_t)(g * 4 + (lane & 3));
  double* yst = stage[wave];

  const double sc = (colscale != nullptr && f0 == sfield) ? colscale[dcl] : 1.0;
  const T* fb = reinterpret_cast<const T*>(fp.p[f0]) + dcl;

  double acc[NA];
#pragma unroll
  for (int a = 0; a < NA; ++a) acc[a] = 0.0;
  double s0N = 0.0, s0S = 0.0, scN = 0.0, scS = 0.0, ssN = 0.0, ssS = 0.0;

  T xb[PD][MB];
  int er[PD][MB];
  double2 wv[PD][MB];
  int fl[PD];
  double ys[TJ];
  auto load_ys = [&](int gi) __attribute__((always_inline)) {
#pragma unroll
    for (int j = 0; j < TJ; ++j) ys[j] = (tab + (int64_t)gi * TE)[(lane + 64 * j) < TE ? (lane + 64 * j) : 0];
  };
  int4 rn;
  // X and weight pairs of batch b, whose indices are rv (the tables are padded).  The weights of an entry do not depend
  // on its index: they go out with the X loads, PD - 1 batches ahead, straight into their slot of the ring.
  auto issue = [&](auto pc, int b, const int4 rv) __attribute__((always_inline)) {
    constexpr int P = decltype(pc)::value;
    er[P][0] = rv.x; er[P][1] = rv.y; er[P][2] = rv.z; er[P][3] = rv.w;
    fl[P] = __builtin_amdgcn_readfirstlane(rv.x) >> 28;
#pragma unroll
    for (int j = 0; j < MB; ++j) wv[P][j] = cw[((int64_t)b * 4 + g) * MB + j];
#pragma unroll
    for (int j = 0; j < MB; ++j) xb[P][j] = TEMX_XLOAD(fb + (int64_t)(er[P][j] & CLS_ROWMASK) * D);
  };
  // the loads of batch b behind the index load of batch b + 1 (which must not queue behind the X loads)
  auto advance = [&](auto pc, int b) __attribute__((always_inline)) {
    const int4 r1 = rn;
    rn = crow[(int64_t)(b + 1) * 4 + g];
    issue(pc, b, r1);
  };
  auto step = [&](auto pc, int b) __attribute__((always_inline)) {
    constexpr int P = decltype(pc)::value;
    if (b + (PD - 1) < b1) advance(std::integral_constant<int, (P + PD - 1) % PD>{}, b + PD - 1);
    const int flags = fl[P] | (b + 1 == b1 ? CLS_LAST : 0);   // a piece may end inside a group: project its partial sums
    if (flags & CLS_SOUTH) {
#pragma unroll
      for (int j = 0; j < MB; ++j) {
        const double x = (double)xb[P][j];
        s0S += (er[P][j] < 0 ? 0.0 : 1.0) * x;          // padding entries read row 0 and weigh nothing
        scS = fma(wv[P][j].x, x, scS);
        ssS = fma(wv[P][j].y, x, ssS);
      }
    } else {
#pragma unroll
      for (int j = 0; j < MB; ++j) {
        const double x = (double)xb[P][j];
        s0N += (er[P][j] < 0 ? 0.0 : 1.0) * x;
        scN = fma(wv[P][j].x, x, scN);
        ssN = fma(wv[P][j].y, x, ssN);
      }
    }
    if (flags & CLS_LAST) {
#pragma unroll
      for (int j = 0; j < TJ; ++j)
        if (lane + 64 * j < TE) yst[lane + 64 * j] = ys[j];
      ++grp;
      load_ys(grp);                           // the table is padded by one group
      const double cE = (scN + scS) * sc, cO = (scN - scS) * sc;
      const double sE = (ssN + ssS) * sc, sO = (ssN - ssS) * sc;
      const double zE = (s0N + s0S) * sc, zO = (s0N - s0S) * sc;
#pragma unroll
      for (int a = 0; a < NA; ++a) {
        const int t = a % NB;
        const double bv = a < NB ? (t < TBS ? cE : cO) : (t < TBS ? sE : sO);
        acc[a] = TEMX_MFMA4(yst[t * 16 + yoff], bv, acc[a]);
      }
#pragma unroll
      for (int a = 0; a < NA; ++a) acc[a] = TEMX_MFMA4(yst[YE + a * 16 + yoff], zE, acc[a]);
#pragma unroll
      for (int a = 0; a < NA; ++a) acc[a] = TEMX_MFMA4(yst[YE + ZE + a * 16 + yoff], zO, acc[a]);
      s0N = s0S = scN = scS = ssN = ssS = 0.0;
    }
  };

  if (b0 < b1) {
    static_assert(PD + 1 <= CLS_PADB, "crow padding must cover the index prefetch");
    load_ys(grp);
    // prologue: X of the first PD - 1 batches (the tables are padded, a short list just loads padding)
    rn = crow[(int64_t)b0 * 4 + g];
    static_for<PD - 1>([&](auto kc) __attribute__((always_inline)) {
      constexpr int k = decltype(kc)::value;
      if (k == 0 || b0 + k < b1) advance(kc, b0 + k);
    });
    for (int b = b0; b < b1; b += PD)
      static_for<PD>([&](auto kc) __attribute__((always_inline)) {
        constexpr int k = decltype(kc)::value;
        if (k == 0 || b + k < b1) step(kc, b + k);
      });
  }

  // (an empty range still stores its zero slab: the reduction sums every slab)
  if (dvalid) {
    const int Kc = 2 * ndeg;
#pragma unroll
    for (int a = 0; a < NA; ++a) {
      const int j = wavecls_acc_col(TBS, ndeg, a, g);
      if (j >= 0) partial[(((int64_t)split * NF + f0) * Kc + j) * D + d] = acc[a];
    }
  }
}

}  // namespace temx
