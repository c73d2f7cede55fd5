// hyisopycnal.h -- IsopycnalSkewSymmetricDiffusivity (Gent-McWilliams plus Redi) of the HydrostaticFreeSurfaceModel, included by
// splitexplicit.hip after hyribased.h (it shares HyMetric, HyBuoy, hy_b, hy_div and the no-contraction rule of that file's kernels).
//
//   reference (paths relative to the reference's src/)                                          here
//   TurbulenceClosures/turbulence_closure_implementations/isopycnal_skew_symmetric_diffusivity.jl
//     :83-108  calculate_diffusivities!, compute_tapered_R33!                                    k_hy_iso_slopes (in update_state!)
//     :130-178 tapering_factor, calc_tapering                                                    hy_iso_taper, k_hy_iso_slopes
//     :186-271 diffusive_flux_x / _y / _z                                                        k_hy_iso_flux
//     :284-289 kappa_z^ccf = eps_R33 kappa_symmetric                                             k_hy_iso_kz (the solve is hyconvect.h's)
//   TurbulenceClosures/isopycnal_rotation_tensor_components.jl:60-122                            k_hy_iso_slopes
//   BuoyancyModels/seawater_buoyancy.jl:119-176, linear_equation_of_state.jl:69-71, buoyancy_tracer.jl:12-16
//   Operators/interpolation_operators.jl:33-68, closure_kernel_operators.jl:43-48
//
// Two forms of the buoyancy gradient occur and each stays where the reference has it: the DIRECT derivative d_x b = g (alpha d_x T -
// beta d_x S) (the component along the face's own direction), and the INTERPOLATED derivative, a difference of the pointwise
// buoyancy_perturbation g (alpha T - beta S) (the two other components).  For a BuoyancyTracer the two are the same expression.
//
// The slopes and the tapering factor depend on the buoyancy alone, so one pass per update_state! stores, with the reference's own
// expressions (the values the fluxes would recompute, bit for bit):
//   eps[i, j, k] = min(eps_fcc, eps_cfc, eps_ccf), all three at the SAME indices (i, j, k), as written;
//   R13 at (Face, Center, Center), R23 at (Center, Face, Center), R31 and R32 at (Center, Center, Face);
//   eps_R33 = eps R33 at (Center, Center, Face), the reference's diffusivity_fields.eps_R33 (faces 1..Nz of the grid's columns).
// All of them live in arrays of the (Center, Center, Face) parent shape, element (i, j, k) at parent (i - 1 + Hx, j - 1 + Hy,
// k - 1 + Hz).  The pass covers i = 1..Nx + 1, j = 1..Ny + 1, k = 1..Nz + 1: the interior plus the column, row and face the east, north
// and top fluxes read.  It reads T and S at i - 1..i + 1, j - 1..j + 1, k - 1..k + 1, that is two halo cells in every direction, and reads
// them exactly as the fills leave them (the y-z edge cells and the cells beyond the first halo cell of a wall are zero).
//
// min and max propagate NaN as Julia's do (fmin / fmax would drop it); every slope division is an IEEE division, so +-Inf and NaN
// pass through: at face 1 and face Nz + 1 the no-flux halo makes d_z b == 0, the slope is +-Inf and eps_ccf == 0 -- or, where the
// horizontal gradient is exactly zero as well, 0 / 0 = NaN, which the reference's tendency then carries.  Ported as written.
struct HyIsoParam {
  double smax2;        // max_slope^2 (FluxTapering)
  double minbz;        // SmallSlopeIsopycnalTensor.minimum_bz
};

OCN_DEVFN double hy_iso_min(double a, double b) { return a != a ? a : (b != b ? b : (b < a ? b : a)); }
OCN_DEVFN double hy_iso_max(double a, double b) { return a != a ? a : (b != b ? b : (b > a ? b : a)); }

// calc_tapering (:169-178); also hands back the clipped bz and the two slopes, which the rotation tensor components share
OCN_DEVFN double hy_iso_taper(double bx, double by, double bz, const HyIsoParam& p, double& bzc, double& sx, double& sy) {
  OCN_NO_CONTRACT
  bzc = hy_iso_max(bz, p.minbz);
  sx = -bx / bzc;
  sy = -by / bzc;
  const double s2 = bzc < 0 ? 0.0 : sx * sx + sy * sy;
  return hy_iso_min(1.0, p.smax2 / s2);
}

// one thread per column (i, j) of i = 1..Nx + 1, j = 1..Ny + 1, marching upwards over faces / levels k = 1..Nz + 1 with the three
// levels k - 1, k, k + 1 of the buoyancy perturbation of its 3 x 3 columns in registers.  T, S: the tracers the buoyancy reads (S null
// for a BuoyancyTracer); dzf_top: dz^f at face Nz + 2 (the grid's table ends at Nz + 1); sy, sz: strides of the tracers; syk, szk: of
// the six outputs
__global__ void __launch_bounds__(256) k_hy_iso_slopes(HyMetric g, HyBuoy q, HyIsoParam p, double dzf_top, const double* __restrict__ T,
                                                       const double* __restrict__ S, double* __restrict__ eps, double* __restrict__ r13,
                                                       double* __restrict__ r23, double* __restrict__ r31, double* __restrict__ r32,
                                                       double* __restrict__ er33, long sy, long sz, long syk, long szk) {
  OCN_NO_CONTRACT
  const int i = blockIdx.x * blockDim.x + threadIdx.x, j = blockIdx.y * blockDim.y + threadIdx.y;
  if (i > g.Nx || j > g.Ny) return;
  const int r = OCN_UNIFORM(j + g.Hy);       // blockDim.x == 64: one row per wave
  const long c0 = (i + g.Hx) + (long)r * sy + (long)(g.Hz - 1) * sz;      // level 0 of the centre column
  long ck = (i + g.Hx) + (long)r * syk + (long)g.Hz * szk;
  // b[l][a][e]: level k - 1 + l, column (i - 1 + a, j - 1 + e); t / s: T and S of the columns the direct derivatives read --
  // [0] (i - 1, j), [1] (i, j - 1), [2] (i, j) -- at levels k - 1 ([.][0]) and k ([.][1])
  double b[3][3][3], t[3][2], s[3][2];
  auto load = [&](int l, long c) {
#pragma unroll
    for (int a = 0; a < 3; ++a)
#pragma unroll
      for (int e = 0; e < 3; ++e) {
        const long cc = c + (a - 1) + (long)(e - 1) * sy;
        b[l][a][e] = hy_b(q, T[cc], S ? S[cc] : 0.0);
      }
  };
  auto load_ts = [&](int m, long c) {
    t[0][m] = T[c - 1]; t[1][m] = T[c - sy]; t[2][m] = T[c];
    s[0][m] = S ? S[c - 1] : 0.0; s[1][m] = S ? S[c - sy] : 0.0; s[2][m] = S ? S[c] : 0.0;
  };
  load(1, c0);
  load(2, c0 + sz);
  load_ts(1, c0);
  const double dxr = g.dxfc[r], dxrm = g.dxfc[r - 1];
  const double dyr = g.dycf[r], dyr1 = g.dycf[r + 1];
  const bool own = i < g.Nx && j < g.Ny;
  for (int k = 1; k <= g.Nz + 1; ++k, ck += szk) {
    // shift the window up one level: levels k - 1, k, k + 1
#pragma unroll
    for (int a = 0; a < 3; ++a)
#pragma unroll
      for (int e = 0; e < 3; ++e) {
        b[0][a][e] = b[1][a][e];
        b[1][a][e] = b[2][a][e];
      }
#pragma unroll
    for (int m = 0; m < 3; ++m) { t[m][0] = t[m][1]; s[m][0] = s[m][1]; }
    const long c = c0 + (long)k * sz;
    load(2, c + sz);
    load_ts(1, c);
    const double dzk = g.dzf[k - 1], dzk1 = k <= g.Nz ? g.dzf[k] : dzf_top;      // dz^f at faces k and k + 1
    // the interpolated derivatives of the buoyancy perturbation: dx at (Face i - 1 + a [a = 1, 2], row e, level l), dy at
    // (column a, Face row j - 1 + e [e = 1, 2], level l), dz at (column a, row e, face k + f [f = 0, 1])
    auto dx = [&](int l, int a, int e) { return (b[l][a][e] - b[l][a - 1][e]) / (e == 0 ? dxrm : dxr); };      // rows j - 1 and j only
    auto dy = [&](int l, int a, int e) { return (b[l][a][e] - b[l][a][e - 1]) / (e == 1 ? dyr : dyr1); };
    auto dz = [&](int f, int a, int e) { return (b[1 + f][a][e] - b[f][a][e]) / (f == 0 ? dzk : dzk1); };
    // the direct derivatives at (i, j, k): seawater_buoyancy.jl:119-176 / buoyancy_tracer.jl:14-16
    double bxd, byd, bzd;
    if (q.kind == 2) {
      bxd = q.g * (q.alpha * ((t[2][1] - t[0][1]) / dxr) - q.beta * ((s[2][1] - s[0][1]) / dxr));
      byd = q.g * (q.alpha * ((t[2][1] - t[1][1]) / dyr) - q.beta * ((s[2][1] - s[1][1]) / dyr));
      bzd = q.g * (q.alpha * ((t[2][1] - t[2][0]) / dzk) - q.beta * ((s[2][1] - s[2][0]) / dzk));
    } else {
      bxd = (t[2][1] - t[0][1]) / dxr;
      byd = (t[2][1] - t[1][1]) / dyr;
      bzd = (t[2][1] - t[2][0]) / dzk;
    }
    double bz1, sx1, sy1, bz2, sx2, sy2, bz3, sx3, sy3;
    // (Face, Center, Center): by = I_y^c I_x^f d_y b, bz = I_z^c I_x^f d_z b, bx direct
    const double e1 = hy_iso_taper(bxd, 0.5 * (0.5 * (dy(1, 0, 1) + dy(1, 1, 1)) + 0.5 * (dy(1, 0, 2) + dy(1, 1, 2))),
                                   0.5 * (0.5 * (dz(0, 0, 1) + dz(0, 1, 1)) + 0.5 * (dz(1, 0, 1) + dz(1, 1, 1))), p, bz1, sx1, sy1);
    // (Center, Face, Center): bx = I_y^f I_x^c d_x b, bz = I_z^c I_y^f d_z b, by direct
    const double e2 = hy_iso_taper(0.5 * (0.5 * (dx(1, 1, 0) + dx(1, 2, 0)) + 0.5 * (dx(1, 1, 1) + dx(1, 2, 1))), byd,
                                   0.5 * (0.5 * (dz(0, 1, 0) + dz(0, 1, 1)) + 0.5 * (dz(1, 1, 0) + dz(1, 1, 1))), p, bz2, sx2, sy2);
    // (Center, Center, Face): bx = I_z^f I_x^c d_x b, by = I_z^f I_y^c d_y b, bz direct
    const double e3 = hy_iso_taper(0.5 * (0.5 * (dx(0, 1, 1) + dx(0, 2, 1)) + 0.5 * (dx(1, 1, 1) + dx(1, 2, 1))),
                                   0.5 * (0.5 * (dy(0, 1, 1) + dy(0, 1, 2)) + 0.5 * (dy(1, 1, 1) + dy(1, 1, 2))), bzd, p, bz3, sx3, sy3);
    const double e = hy_iso_min(hy_iso_min(e1, e2), e3);
    eps[ck] = e;
    r13[ck] = bz1 == 0 ? 0.0 : sx1;
    r23[ck] = bz2 == 0 ? 0.0 : sy2;
    r31[ck] = bz3 == 0 ? 0.0 : sx3;
    r32[ck] = bz3 == 0 ? 0.0 : sy3;
    if (own && k <= g.Nz) er33[ck] = e * (bz3 == 0 ? 0.0 : sx3 * sx3 + sy3 * sy3);
  }
}

// the coefficient field of one tracer's vertically implicit solve over the grid's columns, faces 1..Nz: kappa_symmetric eps_R33, plus
// the kappa of a ConvectiveAdjustmentVerticalDiffusivity / RiBasedVerticalDiffusivity (Face) of the same tuple (vk, or null): the
// tuple's closures are summed on the coefficient, HyCvCol<0> then forms one diagonal term from the sum
__global__ void k_hy_iso_kz(int Nx, int Ny, int Nz, int Hx, int Hy, int Hz, double ks, const double* __restrict__ er33,
                            const double* __restrict__ vk, double* __restrict__ out, long syk, long szk) {
  OCN_NO_CONTRACT
  const int i = blockIdx.x * blockDim.x + threadIdx.x, j = blockIdx.y * blockDim.y + threadIdx.y, k = blockIdx.z;
  if (i >= Nx || j >= Ny || k >= Nz) return;
  const long c = (i + Hx) + (long)(j + Hy) * syk + (long)(k + Hz) * szk;
  const double a = er33[c] * ks;
  out[c] = vk ? a + vk[c] : a;
}

// G_c -= div q of this closure for every tracer of the table at the cell (i, j, k): the six face fluxes from the stored fields and the
// tracer's own neighbourhood (the cell's column and its four neighbours, levels k - 1..k + 1)
#define HY_ISO_MAXT 8
struct HyIsoTracers {
  const double* c[HY_ISO_MAXT];
  double* G[HY_ISO_MAXT];
  double ks[HY_ISO_MAXT], kk[HY_ISO_MAXT];      // kappa_symmetric, kappa_skew
  int n;
};
__global__ void __launch_bounds__(256) k_hy_iso_flux(HyMetric g, HyIsoTracers tr, const double* __restrict__ eps, const double* __restrict__ r13,
                                                     const double* __restrict__ r23, const double* __restrict__ r31,
                                                     const double* __restrict__ r32, long sy, long sz, long syk, long szk) {
  OCN_NO_CONTRACT
  const int i = blockIdx.x * blockDim.x + threadIdx.x, j = blockIdx.y * blockDim.y + threadIdx.y, k = blockIdx.z;
  if (i >= g.Nx || j >= g.Ny) return;
  const int r = OCN_UNIFORM(j + g.Hy);       // blockDim.x == 64: one row per wave
  const long cc = (i + g.Hx) + (long)r * sy + (long)(k + g.Hz) * sz;
  const long ck = (i + g.Hx) + (long)r * syk + (long)(k + g.Hz) * szk;
  const double dz = g.dzc[k];
  const double rV = 1 / (g.azcc[r] * dz);
  const double ax = g.dyfc[r] * dz, ay0 = g.dxcf[r] * dz, ay1 = g.dxcf[r + 1] * dz, az = g.azcc[r];      // Ax^fcc, Ay^cfc at j, j + 1, Az^ccf
  const double e0 = eps[ck], ex = eps[ck + 1], ey = eps[ck + syk], ez = eps[ck + szk];
  const double R13a = r13[ck], R13b = r13[ck + 1], R23a = r23[ck], R23b = r23[ck + syk];
  const double R31a = r31[ck], R31b = r31[ck + szk], R32a = r32[ck], R32b = r32[ck + szk];
  const double dzf0 = g.dzf[k], dzf1 = g.dzf[k + 1], rdzf0 = g.r_dzf[k], rdzf1 = g.r_dzf[k + 1];      // faces k + 1 and k + 2 (0-based k)
  for (int t = 0; t < tr.n; ++t) {
    const double* c = tr.c[t] + cc;
    const double ks = tr.ks[t], kk = tr.kk[t];
    // column m: 0 (i - 1, j), 1 (i, j), 2 (i + 1, j), 3 (i, j - 1), 4 (i, j + 1); level l: k - 1 + l
    double v[5][3];
#pragma unroll
    for (int l = 0; l < 3; ++l) {
      const double* p = c + (long)(l - 1) * sz;
      v[0][l] = p[-1]; v[1][l] = p[0]; v[2][l] = p[1]; v[3][l] = p[-sy]; v[4][l] = p[sy];
    }
    // d_x^fcc c at faces i (a = 0) and i + 1 (a = 1), d_y^cfc c at faces j and j + 1, every level; d_z^ccf c at faces k (f = 0) and k + 1
    double dx[2][3], dy[2][3], dzc[5][2];
#pragma unroll
    for (int l = 0; l < 3; ++l) {
      dx[0][l] = hy_div(v[1][l] - v[0][l], g.dxfc[r], g.r_dxfc[r]);
      dx[1][l] = hy_div(v[2][l] - v[1][l], g.dxfc[r], g.r_dxfc[r]);
      dy[0][l] = hy_div(v[1][l] - v[3][l], g.dycf[r], g.r_dycf[r]);
      dy[1][l] = hy_div(v[4][l] - v[1][l], g.dycf[r + 1], g.r_dycf[r + 1]);
    }
#pragma unroll
    for (int m = 0; m < 5; ++m) {
      dzc[m][0] = hy_div(v[m][1] - v[m][0], dzf0, rdzf0);
      dzc[m][1] = hy_div(v[m][2] - v[m][1], dzf1, rdzf1);
    }
    // I_z^c I_x^f d_z c at faces i, i + 1 and I_z^c I_y^f d_z c at faces j, j + 1
    const double zx0 = 0.5 * (0.5 * (dzc[0][0] + dzc[1][0]) + 0.5 * (dzc[0][1] + dzc[1][1]));
    const double zx1 = 0.5 * (0.5 * (dzc[1][0] + dzc[2][0]) + 0.5 * (dzc[1][1] + dzc[2][1]));
    const double zy0 = 0.5 * (0.5 * (dzc[3][0] + dzc[1][0]) + 0.5 * (dzc[3][1] + dzc[1][1]));
    const double zy1 = 0.5 * (0.5 * (dzc[1][0] + dzc[4][0]) + 0.5 * (dzc[1][1] + dzc[4][1]));
    const double qx0 = -e0 * (ks * dx[0][1] + ((ks - kk) * R13a) * zx0), qx1 = -ex * (ks * dx[1][1] + ((ks - kk) * R13b) * zx1);
    const double qy0 = -e0 * (ks * dy[0][1] + ((ks - kk) * R23a) * zy0), qy1 = -ey * (ks * dy[1][1] + ((ks - kk) * R23b) * zy1);
    // I_z^f I_x^c d_x c and I_z^f I_y^c d_y c at faces k and k + 1; the kappa_symmetric R33 d_z c part is the implicit solve's
    const double xz0 = 0.5 * (0.5 * (dx[0][0] + dx[1][0]) + 0.5 * (dx[0][1] + dx[1][1]));
    const double xz1 = 0.5 * (0.5 * (dx[0][1] + dx[1][1]) + 0.5 * (dx[0][2] + dx[1][2]));
    const double yz0 = 0.5 * (0.5 * (dy[0][0] + dy[1][0]) + 0.5 * (dy[0][1] + dy[1][1]));
    const double yz1 = 0.5 * (0.5 * (dy[0][1] + dy[1][1]) + 0.5 * (dy[0][2] + dy[1][2]));
    const double qz0 = -(e0 * 0.0) - e0 * (((ks + kk) * R31a) * xz0 + ((ks + kk) * R32a) * yz0);
    const double qz1 = -(ez * 0.0) - ez * (((ks + kk) * R31b) * xz1 + ((ks + kk) * R32b) * yz1);
    const double div = rV * (((ax * qx1 - ax * qx0) + (ay1 * qy1 - ay0 * qy0)) + (az * qz1 - az * qz0));
    double* G = tr.G[t] + cc;
    *G = *G - div;
  }
}
