// hywenoz.h -- WENO5(grid = grid) of the hydrostatic model on a vertically stretched grid: the coefficient table, the z
// reconstruction that reads it, and the tracer kernel k_hy_Gc_sz (included from splitexplicit.hip after k_hy_Gc_hi; hymomflux.h uses
// hy_flux_sz for Wu and Wv).
//
// Restated from the reference (paths relative to its src/):
//   Advection/weno_fifth_order.jl:182-209      the tables are those of with_halo((4, 4, 4), grid); x, y, longitude and latitude are
//                                              regular on these grids (:555-556: nothing), and nothing reconstructs at z^aac (w is not
//                                              prognostic), so coeff_z^aaf is the one table that is read
//   Grids/grid_generation.jl:40-48             halo faces of a stretched Bounded coordinate: the boundary cell's width, repeated
//   :562-584, 740-772                          calc_interpolating_coefficients, create_interp_coefficients, interp_weights(r, coord, i, 0, -)
//   :299-305, 493-497, 526-539                 candidates: left p0, p1, p2 take r = 0, 1, 2, right p0, p1, p2 take r = -1, 0, 1, at the
//                                              face's own index
//   :311-317, 380-403                          smoothness indicators (stretched_smoothness = false) and Z weights: those of recon5
//
// Table layout: 12 doubles per face k = 0 .. Nz + 1, [k][r + 1][n], r = -1, 0, 1, 2 the stencil, n = 0, 1, 2 its cells k - r - 1 + n.
#pragma once
#include <vector>

// ---- host: the table ------------------------------------------------------------------------------------------------------------------
// interp_weights(r, coord, i, 0, -) as written; coord(n): the face of reference index n
template <class F>
static void hy_interp_weights(int r, const F& coord, int i, double out[3]) {
  for (int j = 0; j <= 2; ++j) {
    double c = 0;
    for (int m = j + 1; m <= 3; ++m) {
      double num = 0;
      for (int l = 0; l <= 3; ++l) {
        if (l == m) continue;
        double prod = 1;
        for (int q = 0; q <= 3; ++q)
          if (q != m && q != l) prod *= coord(i) - coord(i - (r - q + 1));
        num += prod;
      }
      double den = 1;
      for (int l = 0; l <= 3; ++l)
        if (l != m) den *= coord(i - (r - m + 1)) - coord(i - (r - l + 1));
      c += num / den;
    }
    out[j] = c * (coord(i - (r - j)) - coord(i - (r - j + 1)));
  }
}

// zf: the Nz + 1 interior faces.  Faces 1 - 4 .. Nz + 1 + 4 first (the halo of with_halo((4, 4, 4), grid)), then the four stencils
// of every face 0 .. Nz + 1.
static std::vector<double> hy_weno_table(const std::vector<double>& zf) {
  const int H = 4, n = (int)zf.size() - 1;
  std::vector<double> F(n + 1 + 2 * H);
  const double dm = zf[1] - zf[0], dp = zf[n] - zf[n - 1];
  for (int m = 1; m <= H; ++m) {
    double sm = dm, sp = dp;                     // sum of m copies, left to right
    for (int q = 1; q < m; ++q) { sm += dm; sp += dp; }
    F[H - m] = zf[0] - sm;
    F[H + n + m] = zf[n] + sp;
  }
  for (int k = 0; k <= n; ++k) F[H + k] = zf[k];
  auto coord = [&](int i) { return F[i - 1 + H]; };
  std::vector<double> tab((size_t)(n + 2) * 12);
  for (int i = 0; i <= n + 1; ++i)
    for (int r = -1; r <= 2; ++r) hy_interp_weights(r, coord, i, &tab[(size_t)i * 12 + (r + 1) * 3]);
  return tab;
}

// ---- device ---------------------------------------------------------------------------------------------------------------------------
// recon5<ADV_WENO_Z> (stencils.h) at the face between m1 and c0 with the candidates of the face's table row t: the same smoothness
// indicators and Z weights in the same difference form, the candidate values sum(coeff * psi) as the reference forms them; the fast
// reciprocal still multiplies the weighted sum of candidate DIFFERENCES from the upwind cell.
OCN_DEVFN double recon5_sz(const double* t, double m3, double m2, double m1, double c0, double c1, double c2, bool pos) {
  const double A3 = pos ? m3 : c2, A2 = pos ? m2 : c1, A1 = pos ? m1 : c0, A0 = pos ? c0 : m1, B1 = pos ? c1 : m2;
  const double e1 = A2 - A3, e2 = A1 - A2, e3 = A0 - A1, e4 = B1 - A0;
  const double t0 = e4 - e3, t1 = e3 - e2, t2 = e2 - e1;
  const double s2 = pos ? 2.0 : -2.0;
  const double u0 = fma(-s2, pos ? e3 : e4, t0);
  const double u1 = e2 + e3;
  const double u2 = fma(s2, pos ? e2 : e1, t2);
  const double c3 = 3.0 / 13.0, eps = 1e-6 * (12.0 / 13.0);
  const double d0 = fma(t0, t0, fma(u0 * c3, u0, eps));
  const double d1 = fma(t1, t1, fma(u1 * c3, u1, eps));
  const double d2 = fma(t2, t2, fma(u2 * c3, u2, eps));
  // stencils r = -1: (c0, c1, c2), 0: (m1, c0, c1), 1: (m2, m1, c0), 2: (m3, m2, m1).  In recon5's numbering candidate 0 is the stencil
  // of (A1, A0, B1), 1 of (A2, A1, A0), 2 of (A3, A2, A1): r = 0, 1, 2 for the left-biased form, r = 1, 0, -1 for the right-biased one
  const double q0 = (t[3] * m1 + t[4] * c0) + t[5] * c1;
  const double q1 = (t[6] * m2 + t[7] * m1) + t[8] * c0;
  const double qo = pos ? (t[9] * m3 + t[10] * m2) + t[11] * m1 : (t[0] * c0 + t[1] * c1) + t[2] * c2;
  const double r0 = 3.0 * ((pos ? q0 : q1) - A1), r1 = 6.0 * ((pos ? q1 : q0) - A1), r2 = qo - A1;
  const double w0 = d0 * d0, w1 = d1 * d1, w2 = d2 * d2;
  const double P0 = w1 * w2, P1 = w0 * w2, P2 = w0 * w1;
  const double tau = d2 - d0, tt = tau * tau, Q = w0 * P0;
  const double a0 = fma(tt, P0, Q), a1 = fma(tt, P1, Q), a2 = fma(tt, P2, Q);
  const double num = fma(a0, r0, fma(a1, r1, a2 * r2));
  const double den = fma(3.0, a0, fma(6.0, a1, a2));
  return fma(num, fast_rcp(den), A1);
}

// adv_flux_b<ADV_WENO_Z> along z from memory with the table row t of the face kf (1-based) between p[-s] and p[0]
OCN_DEVFN double hy_flux_sz(const double* p, long s, double ut, int kf, int Nz, const double* t) {
  const bool pos = ut > 0.0;
  if (!(pos ? outside_left(kf, Nz, 2) : outside_right(kf, Nz, 2))) return ut * sym2(p - s, s);
  return ut * recon5_sz(t, p[-3 * s], p[-2 * s], p[-s], p[0], p[s], p[2 * s], pos);
}

// k_hy_Gc_hi<ADV_WENO_Z, NT> with the stretched z reconstruction, as a column march that keeps the six z neighbours c[k-2 .. k+3] of
// the upper face of level k in registers per tracer: one new load per level instead of six per face.  The level index is the same
// in every lane, so a face's twelve coefficients are scalar loads.  x and y fluxes, the boundary buffer and the latitude bands' global
// row are k_hy_Gc_hi's.
template <int NT>
__global__ void __launch_bounds__(256) k_hy_Gc_sz(HyMetric g, const double* __restrict__ u, const double* __restrict__ v,
                                                  const double* __restrict__ w, const double* __restrict__ c0, const double* __restrict__ c1,
                                                  double* __restrict__ G0, double* __restrict__ G1, const double* __restrict__ tab, int xb,
                                                  int yb, int jrow0, int gNy, long syu, long szu, long syv, long szv, long syc, long szc) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x, j = blockIdx.y * blockDim.y + threadIdx.y;
  if (i >= g.Nx || j >= g.Ny) return;
  constexpr int ADV = ADV_WENO_Z, NB = 2;
  const int r = OCN_UNIFORM(j + g.Hy);       // blockDim.x == 64: one row per wave
  long cu = (i + g.Hx) + (long)r * syu + (long)g.Hz * szu, cv = (i + g.Hx) + (long)r * syv + (long)g.Hz * szv;
  long cc = (i + g.Hx) + (long)r * syc + (long)g.Hz * szc;
  const double dyfc = g.dyfc[r], dxcf0 = g.dxcf[r], dxcf1 = g.dxcf[r + 1], azcc = g.azcc[r];
  const int jg = jrow0 + j;
  double fz0[NT], W[NT][6];                  // W: levels k - 3 .. k + 2 before the level's shift, k - 2 .. k + 3 after it
  {
    const double az0 = azcc * w[cc];
#pragma unroll
    for (int t = 0; t < NT; ++t) {
      const double* c = (t ? c1 : c0) + cc;
      W[t][0] = 0.0;
#pragma unroll
      for (int q = 1; q < 6; ++q) W[t][q] = c[(q - 3) * szc];
      fz0[t] = az0 * (0.5 * (W[t][2] + W[t][3]));      // face 1 lies inside the buffer
    }
  }
  for (int k = 0; k < g.Nz; ++k, cu += szu, cv += szv, cc += szc) {
    const double dz = g.dzc[k];
    const double ax0 = (dyfc * dz) * u[cu], ax1 = (dyfc * dz) * u[cu + 1];
    const double ay0 = (dxcf0 * dz) * v[cv], ay1 = (dxcf1 * dz) * v[cv + syv];
    const double az1 = azcc * w[cc + szc];
    const double rv = 1 / (azcc * dz);
    const int kf = OCN_UNIFORM(k + 2);                   // the level's upper face
    const double* tk = tab + 12 * kf;
    double tc[12];
#pragma unroll
    for (int q = 0; q < 12; ++q) tc[q] = tk[q];
    const bool pos = az1 > 0.0;
    const bool hi = pos ? outside_left(kf, g.Nz, NB) : outside_right(kf, g.Nz, NB);
#pragma unroll
    for (int t = 0; t < NT; ++t) {
      const double* c = (t ? c1 : c0) + cc;
#pragma unroll
      for (int q = 0; q < 5; ++q) W[t][q] = W[t][q + 1];
      W[t][5] = c[3 * szc];
      const double fx0 = adv_flux_b<ADV>(c, 1, ax0, xb != 0, i + 1, g.Nx, NB), fx1 = adv_flux_b<ADV>(c + 1, 1, ax1, xb != 0, i + 2, g.Nx, NB);
      const double fy0 = adv_flux_b<ADV>(c, syc, ay0, yb != 0, jg + 1, gNy, NB), fy1 = adv_flux_b<ADV>(c + syc, syc, ay1, yb != 0, jg + 2, gNy, NB);
      double fz1;
      if (hi) fz1 = az1 * recon5_sz(tc, W[t][0], W[t][1], W[t][2], W[t][3], W[t][4], W[t][5], pos);
      else fz1 = az1 * (0.5 * (W[t][2] + W[t][3]));
      (t ? G1 : G0)[cc] = -(rv * (((fx1 - fx0) + (fy1 - fy0)) + (fz1 - fz0[t])));
      fz0[t] = fz1;
    }
  }
}
