// background.hip -- BackgroundFields of the NonhydrostaticModel: the two advection terms that couple the model's fields to
// prescribed background velocities (U, V, W) and background tracers.
//
// Reference (paths relative to the reference's src):
//   Models/NonhydrostaticModels/nonhydrostatic_tendency_kernel_functions.jl:61-63,118-120,172-174,226-228
//   Advection/momentum_advection_operators.jl:20-41,52-86, tracer_advection_operators.jl:8-15,31-35
//   Fields/background_fields.jl:5-75 (members are FunctionFields at the nodes of the field they belong to, halo nodes included)
//
// For u, v, w and every tracer phi, with Phi the background of phi:
//     G_phi  +=  - div(adv, (U, V, W), phi)  -  div(adv, (u, v, w), Phi)
// with the model's own advection scheme and boundary buffers; the upwind bias follows the sign of the ADVECTING velocity -- the
// interpolated background velocity in the first term, the interpolated model velocity in the second.  An absent member is the
// reference's ZeroField: a null pointer whose fluxes are skipped (0 * reconstruction there).  The fluxes are those of k_tend_uvw
// and k_tend_c (kernels.hip), argument for argument, with the advecting or the advected array exchanged for a background member.
//
// A member comes in one of two forms (internal.h bg_*):
//   column -- a table over the parent levels of its field (halo levels included), constant in x and y: strides (0, 0, 1).  k is
//             uniform over the workgroup, so its values are scalar loads; along x and y its symmetric interpolation and every
//             reconstruction of it is the value itself, and the upwind direction it gives the x / y fluxes of the first term
//             is wave-uniform.  What is left per lane: the x / y reconstructions of the model's own field, the x / y
//             differences of the interpolated model velocities times the profile, and the z fluxes, whose reconstruction of the
//             profile follows the lane's own w.
//   field  -- an array in the layout of the parent array of its field: strides (1, sy, sz), read like the model's fields.
// The launches add to G^n after the general tendency kernels or k_rest4 have written it and before anything consumes it
// (kernels.hip launch_tendencies), inside the captured step graphs.
#include "internal.h"

// what a launch reads of one member: the entry of the first interior cell and the strides; p == null: absent
struct BgMem {
  const double* p;
  long sx, sy, sz;
};
struct BgVel {
  BgMem m[3];
};

// ---- views: one array at the cell (i, j, k) of the thread, addressed by cell offsets ------------------------------------------
// KIND 0: a model field (1, g.sy, g.sz); 1: a column table (0, 0, 1), known at compile time; 2: a member with the strides it brings
template <int KIND>
struct BgView {
  static constexpr bool column = KIND == 1;
  const double* c;   // at this cell; null: absent
  long rx, ry, rz;
  OCN_DEVFN long stride(int axis) const {
    if (KIND == 0) return axis == 0 ? 1 : axis == 1 ? ry : rz;
    if (KIND == 1) return axis == 2 ? 1 : 0;
    return axis == 0 ? rx : axis == 1 ? ry : rz;
  }
  OCN_DEVFN const double* at(int di, int dj, int dk) const { return c + di * stride(0) + dj * stride(1) + dk * stride(2); }
  // the value at a cell offset; a column's is the same in every lane: a scalar load
  OCN_DEVFN double val(int di, int dj, int dk) const { return column ? OCN_SLOAD(at(0, 0, dk)) : *at(di, dj, dk); }
};

template <int KIND>
OCN_DEVFN BgView<KIND> bg_view(const BgMem& b, int i, int j, int k) {
  BgView<KIND> v;
  v.rx = b.sx; v.ry = b.sy; v.rz = b.sz;
  v.c = b.p ? b.p + i * v.stride(0) + j * v.stride(1) + k * v.stride(2) : nullptr;
  return v;
}
OCN_DEVFN BgView<0> bg_model_view(const double* p, const GridDev& g, long c) {
  BgView<0> v;
  v.rx = 1; v.ry = g.sy; v.rz = g.sz;
  v.c = p + c;
  return v;
}

// adv_flux_b through the face between the cells (di, dj, dk) - e_AXIS and (di, dj, dk) of q
template <int ADV, int AXIS, class Q>
OCN_DEVFN double bg_flux(const Q& q, int di, int dj, int dk, double ut, bool bounded, int idx, int N, int nb) {
  if (Q::column && AXIS != 2) return ut * q.val(0, 0, dk);   // a profile reconstructed along x or y, by any scheme: the profile
  return adv_flux_b<ADV>(q.at(di, dj, dk), q.stride(AXIS), ut, bounded, idx, N, nb);
}
// sym_b midway between the cells (di, dj, dk) and (di, dj, dk) + e_AXIS of a
template <int ADV, int AXIS, class A>
OCN_DEVFN double bg_sym(const A& a, int di, int dj, int dk, bool bounded, int idx, int N, int nb) {
  if (A::column && AXIS != 2) return a.val(0, 0, dk);
  return sym_b<ADV>(a.at(di, dj, dk), a.stride(AXIS), bounded, idx, N, nb);
}

// the thread's cell: 1-based indices of the reference's boundary-buffer tests, walls, metrics (as k_tend_uvw)
struct BgCell {
  int k, ii, jj, kk, Nx, Ny, Nz, nb;
  bool xb, yb, zb, zf;
  double rdx, rdy, rdzc, rdzf;
};
template <bool WALLS>
OCN_DEVFN BgCell bg_cell(const GridDev& g, int i, int j, int k) {
  BgCell x;
  x.k = k; x.ii = i + 1; x.jj = j + 1; x.kk = k + 1;
  x.Nx = g.Nx; x.Ny = g.Ny; x.Nz = g.Nz; x.nb = g.nb;
  x.xb = WALLS && g.xb != 0; x.yb = WALLS && g.yb != 0; x.zb = g.zb != 0; x.zf = g.zflat != 0;
  x.rdx = g.rdx; x.rdy = g.rdy;
  x.rdzc = x.zf ? 0.0 : g_rdzc(g, k);
  x.rdzf = x.zf ? 0.0 : g_rdzf(g, k);
  return x;
}

// ---- div_vu at fcc (momentum_advection_operators.jl:52-56; k_tend_uvw's Fuu, Fvu, Fwu): acc -= div(adv, (U, V, W), q) -------------
template <int ADV, class A, class Q>
OCN_DEVFN void bg_div_u(const BgCell& x, const A& U, const A& V, const A& W, const Q& q, double& acc) {
  double fx = 0, fy = 0;
  if (U.c) {   // ccc
    auto F = [&](int di, int i1) {
      return bg_flux<ADV, 0>(q, di + 1, 0, 0, bg_sym<ADV, 0>(U, di, 0, 0, x.xb, i1, x.Nx, x.nb), x.xb, i1, x.Nx, x.nb);
    };
    fx = F(0, x.ii) - F(-1, x.ii - 1);
  }
  if (V.c) {   // ffc
    auto F = [&](int dj, int j1) {
      return bg_flux<ADV, 1>(q, 0, dj, 0, bg_sym<ADV, 0>(V, -1, dj, 0, x.xb, x.ii, x.Nx, x.nb), x.yb, j1, x.Ny, x.nb);
    };
    fy = F(1, x.jj + 1) - F(0, x.jj);
  }
  acc -= fx * x.rdx + fy * x.rdy;
  if (!x.zf && W.c) {   // fcf
    auto F = [&](int dk, int k1) {
      return bg_flux<ADV, 2>(q, 0, 0, dk, bg_sym<ADV, 0>(W, -1, 0, dk, x.xb, x.ii, x.Nx, x.nb), x.zb, k1, x.Nz, x.nb);
    };
    acc -= (F(1, x.kk + 1) - F(0, x.kk)) * x.rdzc;
  }
}

// ---- div_vv at cfc (:68-72; Fuv, Fvv, Fwv) ----------------------------------------------------------------------------------------
template <int ADV, class A, class Q>
OCN_DEVFN void bg_div_v(const BgCell& x, const A& U, const A& V, const A& W, const Q& q, double& acc) {
  double fx = 0, fy = 0;
  if (U.c) {   // ffc
    auto F = [&](int di, int i1) {
      return bg_flux<ADV, 0>(q, di, 0, 0, bg_sym<ADV, 1>(U, di, -1, 0, x.yb, x.jj, x.Ny, x.nb), x.xb, i1, x.Nx, x.nb);
    };
    fx = F(1, x.ii + 1) - F(0, x.ii);
  }
  if (V.c) {   // ccc
    auto F = [&](int dj, int j1) {
      return bg_flux<ADV, 1>(q, 0, dj + 1, 0, bg_sym<ADV, 1>(V, 0, dj, 0, x.yb, j1, x.Ny, x.nb), x.yb, j1, x.Ny, x.nb);
    };
    fy = F(0, x.jj) - F(-1, x.jj - 1);
  }
  acc -= fx * x.rdx + fy * x.rdy;
  if (!x.zf && W.c) {   // cff
    auto F = [&](int dk, int k1) {
      return bg_flux<ADV, 2>(q, 0, 0, dk, bg_sym<ADV, 1>(W, 0, -1, dk, x.yb, x.jj, x.Ny, x.nb), x.zb, k1, x.Nz, x.nb);
    };
    acc -= (F(1, x.kk + 1) - F(0, x.kk)) * x.rdzc;
  }
}

// ---- div_vw at ccf (:82-86; Fuw, Fvw, Fww) ----------------------------------------------------------------------------------------
// advecting u, v interpolated in z to the w level; CenteredSecondOrder interpolates the area-weighted velocity (k_tend_uvw's uz)
template <int ADV, class A>
OCN_DEVFN double bg_uz(const GridDev& g, const BgCell& x, const A& a, int di, int dj) {
  if (x.zf) return a.val(di, dj, 0);
  if (ADV == ADV_C2 && g.dzc) return 0.5 * (g_dzc(g, x.k - 1) * a.val(di, dj, -1) + g_dzc(g, x.k) * a.val(di, dj, 0)) * x.rdzf;
  return sym_b<ADV>(a.at(di, dj, -1), a.stride(2), x.zb, x.kk, x.Nz, x.nb);
}
template <int ADV, class A, class Q>
OCN_DEVFN void bg_div_w(const GridDev& g, const BgCell& x, const A& U, const A& V, const A& W, const Q& q, double& acc) {
  double fx = 0, fy = 0;
  if (U.c) {   // fcf
    auto F = [&](int di, int i1) { return bg_flux<ADV, 0>(q, di, 0, 0, bg_uz<ADV>(g, x, U, di, 0), x.xb, i1, x.Nx, x.nb); };
    fx = F(1, x.ii + 1) - F(0, x.ii);
  }
  if (V.c) {   // cff
    auto F = [&](int dj, int j1) { return bg_flux<ADV, 1>(q, 0, dj, 0, bg_uz<ADV>(g, x, V, 0, dj), x.yb, j1, x.Ny, x.nb); };
    fy = F(1, x.jj + 1) - F(0, x.jj);
  }
  acc -= fx * x.rdx + fy * x.rdy;
  if (!x.zf && W.c) {   // ccc
    auto F = [&](int dk, int k1) {
      return bg_flux<ADV, 2>(q, 0, 0, dk + 1, bg_sym<ADV, 2>(W, 0, 0, dk, x.zb, k1, x.Nz, x.nb), x.zb, k1, x.Nz, x.nb);
    };
    acc -= (F(0, x.kk) - F(-1, x.kk - 1)) * x.rdzf;
  }
}

// ---- div_Uc at ccc (tracer_advection_operators.jl:31-35; k_tend_c's Fx, Fy, Fz): the advecting velocity un-interpolated -----------
template <int ADV, class A, class Q>
OCN_DEVFN void bg_div_c(const BgCell& x, const A& U, const A& V, const A& W, const Q& q, double& acc) {
  double fx = 0, fy = 0;
  if (U.c) fx = bg_flux<ADV, 0>(q, 1, 0, 0, U.val(1, 0, 0), x.xb, x.ii + 1, x.Nx, x.nb) - bg_flux<ADV, 0>(q, 0, 0, 0, U.val(0, 0, 0), x.xb, x.ii, x.Nx, x.nb);
  if (V.c) fy = bg_flux<ADV, 1>(q, 0, 1, 0, V.val(0, 1, 0), x.yb, x.jj + 1, x.Ny, x.nb) - bg_flux<ADV, 1>(q, 0, 0, 0, V.val(0, 0, 0), x.yb, x.jj, x.Ny, x.nb);
  acc -= fx * x.rdx + fy * x.rdy;
  if (!x.zf && W.c)
    acc -= (bg_flux<ADV, 2>(q, 0, 0, 1, W.val(0, 0, 1), x.zb, x.kk + 1, x.Nz, x.nb) - bg_flux<ADV, 2>(q, 0, 0, 0, W.val(0, 0, 0), x.zb, x.kk, x.Nz, x.nb)) * x.rdzc;
}

// ---- the two launches ---------------------------------------------------------------------------------------------------------------
// FORM 0: every present member is a column table (compile-time strides, scalar loads); 1: members bring their strides
template <int ADV, bool WALLS, int FORM>
__global__ void k_bg_uvw(GridDev g, BgVel b, const double* __restrict__ u, const double* __restrict__ v,
                         const double* __restrict__ w, double* __restrict__ Gu, double* __restrict__ Gv, double* __restrict__ Gw) {
  int i, j;
  ocn_cell_ij(i, j);
  const int k = blockIdx.z;   // one level per workgroup: k is wave-uniform
  if (i >= g.Nx || j >= g.Ny || k >= g.Nz) return;
  const long c = i + j * g.sy + k * g.sz;
  const BgCell x = bg_cell<WALLS>(g, i, j, k);
  constexpr int KB = FORM == 0 ? 1 : 2;
  const BgView<KB> U = bg_view<KB>(b.m[0], i, j, k), V = bg_view<KB>(b.m[1], i, j, k), W = bg_view<KB>(b.m[2], i, j, k);
  const BgView<0> mu = bg_model_view(u, g, c), mv = bg_model_view(v, g, c), mw = bg_model_view(w, g, c);
  double gu = 0, gv = 0, gw = 0;
  if (U.c || V.c || W.c) {   // div(adv, ::ZeroU, phi) = 0
    bg_div_u<ADV>(x, U, V, W, mu, gu);
    bg_div_v<ADV>(x, U, V, W, mv, gv);
    bg_div_w<ADV>(g, x, U, V, W, mw, gw);
  }
  if (U.c) bg_div_u<ADV>(x, mu, mv, mw, U, gu);   // div(adv, (u, v, w), ::ZeroField) = 0
  if (V.c) bg_div_v<ADV>(x, mu, mv, mw, V, gv);
  if (W.c) bg_div_w<ADV>(g, x, mu, mv, mw, W, gw);
  Gu[c] += gu;
  Gv[c] += gv;
  Gw[c] += gw;
}

struct BgTracers {
  const double* q[OCN_MAX_TRACERS];
  double* G[OCN_MAX_TRACERS];
  BgMem B[OCN_MAX_TRACERS];
  int n;
};

// every tracer of the model in one launch.  FV / FT: the FORM of the background velocities / of the background tracers
template <int ADV, bool WALLS, int FV, int FT>
__global__ void k_bg_c(GridDev g, BgVel b, BgTracers T, const double* __restrict__ u, const double* __restrict__ v,
                       const double* __restrict__ w) {
  int i, j;
  ocn_cell_ij(i, j);
  const int k = blockIdx.z;
  if (i >= g.Nx || j >= g.Ny || k >= g.Nz) return;
  const long c = i + j * g.sy + k * g.sz;
  const BgCell x = bg_cell<WALLS>(g, i, j, k);
  constexpr int KV = FV == 0 ? 1 : 2, KT = FT == 0 ? 1 : 2;
  const BgView<KV> U = bg_view<KV>(b.m[0], i, j, k), V = bg_view<KV>(b.m[1], i, j, k), W = bg_view<KV>(b.m[2], i, j, k);
  const BgView<0> mu = bg_model_view(u, g, c), mv = bg_model_view(v, g, c), mw = bg_model_view(w, g, c);
  const bool vel = U.c || V.c || W.c;
  for (int t = 0; t < T.n; ++t) {
    const BgView<KT> B = bg_view<KT>(T.B[t], i, j, k);
    if (!vel && !B.c) continue;
    double gc = 0;
    if (vel) bg_div_c<ADV>(x, U, V, W, bg_model_view(T.q[t], g, c), gc);
    if (B.c) bg_div_c<ADV>(x, mu, mv, mw, B, gc);
    T.G[t][c] += gc;
  }
}

// what the kernels read of member f in the current stage
static BgMem bg_member(const ocn_model* m, int f) {
  BgMem b = {nullptr, 0, 0, 0};
  if (m->bg_col >> f & 1u) {
    b.p = m->bg_tab.slot(m->stage - 1, m->bg_ci[f]) + m->gd.Hz;
    b.sz = 1;
  } else if ((m->bg_fld >> f & 1u) && m->bg_arr[f]) {
    const Field& F = bg_field_of(m, f);
    b.p = m->bg_arr[f] + (F.interior() - F.d);
    b.sx = 1; b.sy = F.sy; b.sz = F.sz;
  }
  return b;
}

void launch_background(ocn_model* m) {
  if (!model_background(m) || m->d.advection == ADV_NONE) return;   // advection = nothing: every div is zero
  ProfScope ps(m->ctx, "background");
  const GridDev& g = m->gd;
  hipStream_t s = m->ctx->stream;
  BgVel b;
  for (int f = 0; f < 3; ++f) b.m[f] = bg_member(m, f);
  const bool vel = b.m[0].p || b.m[1].p || b.m[2].p;
  const int fv = (m->bg_fld & 7u) ? 1 : 0, ft = (m->bg_fld >> 3) ? 1 : 0;
  BgTracers T;
  T.n = 0;
  bool any_tracer = false;
  for (int t = 0; t < m->nt; ++t) {
    T.q[T.n] = m->tr[t].interior();
    T.G[T.n] = m->Gn[3 + t].interior();
    T.B[T.n] = bg_member(m, 3 + t);
    any_tracer = any_tracer || T.B[T.n].p;
    ++T.n;
  }
  static const dim3 blk(64, 4, 1);
  const dim3 grd((g.Nx + blk.x - 1) / blk.x, (g.Ny + blk.y - 1) / blk.y, g.Nz);
  const double *u = m->u.interior(), *v = m->v.interior(), *w = m->w.interior();
  double *Gu = m->Gn[0].interior(), *Gv = m->Gn[1].interior(), *Gw = m->Gn[2].interior();
  const bool do_uvw = vel, do_c = T.n > 0 && (vel || any_tracer);
#define BG_C(A, W, FVV) { if (ft) ocn_launch(k_bg_c<A, W, FVV, 1>, grd, blk, s, g, b, T, u, v, w); \
                          else ocn_launch(k_bg_c<A, W, FVV, 0>, grd, blk, s, g, b, T, u, v, w); }
#define BG_LAUNCH(A, W)                                                                        \
  if (do_uvw) {                                                                                \
    ProfScope p1(m->ctx, "background_uvw");                                                    \
    if (fv) ocn_launch(k_bg_uvw<A, W, 1>, grd, blk, s, g, b, u, v, w, Gu, Gv, Gw);             \
    else ocn_launch(k_bg_uvw<A, W, 0>, grd, blk, s, g, b, u, v, w, Gu, Gv, Gw);                \
  }                                                                                            \
  if (do_c) {                                                                                  \
    ProfScope p2(m->ctx, "background_c");                                                      \
    if (fv) BG_C(A, W, 1) else BG_C(A, W, 0)                                                   \
  }
#define BG_CASE(A)              \
  case A:                       \
    if (g.xb || g.yb) {         \
      BG_LAUNCH(A, true)        \
    } else {                    \
      BG_LAUNCH(A, false)       \
    }                           \
    break;
  switch (m->d.advection) {
    BG_CASE(ADV_C2)
    BG_CASE(ADV_C4)
    BG_CASE(ADV_U5)
    BG_CASE(ADV_WENO_Z)
    BG_CASE(ADV_WENO_JS)
    BG_CASE(ADV_U1)
    BG_CASE(ADV_U3)
    default: break;
  }
#undef BG_CASE
#undef BG_LAUNCH
#undef BG_C
}
