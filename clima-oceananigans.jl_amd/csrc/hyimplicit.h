// hyimplicit.h -- ImplicitFreeSurface(solver_method = :PreconditionedConjugateGradient, preconditioner = nothing) of the hydrostatic
// model (included by splitexplicit.hip).
//
//   reference (paths relative to its src/)                                                      here
//   Models/HydrostaticFreeSurfaceModels/implicit_free_surface.jl:125-160 (implicit_free_surface_step!)   ifs_solve
//   .../compute_vertically_integrated_variables.jl (sum!(∫ᶻQ.u, Ax * u), sum!(∫ᶻA, Ax))          k_hy_momentum_ifs, k_ifs_vsum,
//                                                                                                 ocn_ifs_create
//   .../pcg_implicit_free_surface_solver.jl:116-120 (right-hand side), :130-180 (L(η))           k_ifs_init, k_ifs_pq
//   Solvers/preconditioned_conjugate_gradient_solver.jl:132-236 (solve!, iterate!, iterating)    k_ifs_pq, k_ifs_xr, ifs_solve
//   .../barotropic_pressure_correction.jl:20-33,44-50 (u -= g Δt ∂x η, v -= g Δt ∂y η)           k_ifs_correct
//
// The solve.  The 2-D problem is small (config 5: 0.5 M cells, 4 MB per field) and the iteration is a chain of dependent reductions,
// so its cost is launches and reductions, not bandwidth.  One iteration is two launches:
//   k_ifs_pq  re-reduces the partials of r·r (‖r‖, ρ, the stop test), forms p = r + β p_old at every parent cell *as the halo fill would
//             leave it* (a halo cell reads the cell its fill copies), writes p into the other buffer of a pair, q = L(p) over the
//             interior, and one partial of p·q per block;
//   k_ifs_xr  re-reduces the partials of p·q (α = ρ / p·q), x += α p and r -= α q over the parent array, one partial of r·r per block.
// Every block reduces the few hundred partials of the previous launch itself, in one fixed order, so no launch finishes a reduction
// and nothing needs a fence or an atomic; the sums (and with them the iterates) are the same bits run after run, on either step path
// and on every rank.  The scalars live in IfsState on the device.  A launch reads only state words that the OTHER kernel writes, so no
// block sees a word change under it.  After the stop test has fired every launch returns at once; the host launches the iterations in
// batches and reads the stop flag once per batch.
//
// Parent-array semantics as the reference's: r, p and x are updated over the whole parent array (pp .= zp .+ β pp, xp .+= α pp,
// rp .-= α qp), the halos of r and q stay zero (b and q are written over the interior only), and the fill of p that L performs
// first is folded into the formation of p.  The arithmetic is compiled without contraction (the reference's broadcasts do not fuse).
#pragma once

#define IFS_NT 1024       // threads per block of the solver kernels (sixteen waves: four per SIMD, for the latency of the loads)
#define IFS_NBMAX 256     // blocks of the solver kernels at most (one per CU): the partials every block re-reduces

struct IfsState {
  int it;            // iterations done (k_ifs_xr writes it)
  int itA;           // the iteration k_ifs_pq is working on (k_ifs_pq writes it)
  int stop;          // the stop test fired in an earlier iteration (k_ifs_xr writes it)
  int stopA;         // the stop test fired (k_ifs_pq writes it)
  int nonfinite;     // ‖r‖ was not finite
  int pad;
  double tol, rnorm; // tolerance of this solve; ‖r‖ at the stop test
  double rho[2];     // ρ of iteration n in slot n & 1
};

// the Center-Center parent array of the solver's fields, and the fill order of hfield_fill
struct IfsGeo {
  int Nx, Ny, Hx, Hy, Tx, Ty;
  int xper, yper, yfirst;      // Periodic x / y; the fill does y before x (x Periodic, y Bounded)
  long su, sv;                 // row strides of the (Face, Center) and (Center, Face) arrays
};

struct IfsOp {
  const double *Ax, *Ay;       // ∫ᶻ Ax at (Face, Center), ∫ᶻ Ay at (Center, Face), halos filled
  const double *dxfc, *dycf, *azcc;
  const double *r_dxfc, *r_dycf;   // correctly rounded reciprocals: the divisions are hy_div's (IEEE quotients in three instructions)
  double gdt2, r_gdt2;         // g Δt^2 and its correctly rounded reciprocal
};

// ---- the parent cell whose value the halo fill copies into (i, j) ---------------------------------------------------------------
// hfield_fill of a (Center, Center, Nothing) field: Bounded -> the first halo cell copies the edge cell, over the interior cells of
// the other direction; Periodic -> the halo copies the far interior, over the whole extent of the other direction (N >= H).  Two fills
// compose: the value at (i, j) after both is the value at map_first(map_last(i, j)) before them.
__device__ inline void ifs_map_x(const IfsGeo& g, int& i, int j) {
  if (g.xper) {
    if (i < g.Hx) i += g.Nx;
    else if (i >= g.Hx + g.Nx) i -= g.Nx;
  } else if (j >= g.Hy && j < g.Hy + g.Ny) {
    if (i == g.Hx - 1) i = g.Hx;
    else if (i == g.Hx + g.Nx) i = g.Hx + g.Nx - 1;
  }
}
__device__ inline void ifs_map_y(const IfsGeo& g, int i, int& j) {
  if (g.yper) {
    if (j < g.Hy) j += g.Ny;
    else if (j >= g.Hy + g.Ny) j -= g.Ny;
  } else if (i >= g.Hx && i < g.Hx + g.Nx) {
    if (j == g.Hy - 1) j = g.Hy;
    else if (j == g.Hy + g.Ny) j = g.Hy + g.Ny - 1;
  }
}
__device__ inline long ifs_src(const IfsGeo& g, int i, int j) {
  if (g.yfirst) {       // fills y then x: undo x first
    ifs_map_x(g, i, j);
    ifs_map_y(g, i, j);
  } else {
    ifs_map_y(g, i, j);
    ifs_map_x(g, i, j);
  }
  return i + (long)j * g.Tx;
}

// ---- deterministic sums ---------------------------------------------------------------------------------------------------------
// A wave sums its 64 lanes by a butterfly: at every stage lane l and lane l ^ m add the same two numbers (in either order: the same
// bits), so every lane ends with the same sum.  A block's partial is the sum of its waves' sums, in wave order.  The total of the
// partials: lane l of wave 0 sums partials l, l + 64, ... in order, then the butterfly.  The host emulation runs a block's threads
// one after another (compat.h): the last thread forms the block's partial and the first the total, in exactly these orders.
#ifndef OCN_HOST_EMU
__device__ inline double ifs_wave_sum(double v) {
  for (int m = 32; m >= 1; m >>= 1) v = v + __shfl_xor(v, m, 64);
  return v;
}
// every thread of the block calls it; thread 0 writes the block's partial
__device__ inline void ifs_block_partial(double acc, double* part) {
  OCN_SHARED double w[IFS_NT / 64];
  const int t = threadIdx.x;
  const double s = ifs_wave_sum(acc);
  if ((t & 63) == 0) w[t >> 6] = s;
  __syncthreads();
  if (t == 0) {
    double b = w[0];
    for (int q = 1; q < IFS_NT / 64; ++q) b = b + w[q];
    part[blockIdx.x] = b;
  }
}
// every thread of the block calls it and receives the total of the nb partials
__device__ inline double ifs_total(const double* part, int nb) {
  OCN_SHARED double tot;
  const int t = threadIdx.x;
  if (t < 64) {
    double s = 0.0;
    for (int q = t; q < nb; q += 64) s = s + part[q];
    s = ifs_wave_sum(s);
    if (t == 0) tot = s;
  }
  __syncthreads();
  const double r = tot;
  __syncthreads();       // tot is written again by the next call
  return r;
}
#else
static inline void ifs_butterfly(double* v) {
  double t[64];
  for (int m = 32; m >= 1; m >>= 1) {
    for (int l = 0; l < 64; ++l) t[l] = v[l] + v[l ^ m];
    for (int l = 0; l < 64; ++l) v[l] = t[l];
  }
}
static inline void ifs_block_partial(double acc, double* part) {
  static double lanes[IFS_NT];
  const int t = threadIdx.x;
  lanes[t] = acc;
  if (t != IFS_NT - 1) return;
  double w[IFS_NT / 64];
  for (int q = 0; q < IFS_NT / 64; ++q) {
    double v[64];
    for (int l = 0; l < 64; ++l) v[l] = lanes[64 * q + l];
    ifs_butterfly(v);
    w[q] = v[0];
  }
  double b = w[0];
  for (int q = 1; q < IFS_NT / 64; ++q) b = b + w[q];
  part[blockIdx.x] = b;
}
static inline double ifs_total(const double* part, int nb) {
  static double tot;
  if (threadIdx.x == 0) {
    double v[64];
    for (int l = 0; l < 64; ++l) {
      double s = 0.0;
      for (int q = l; q < nb; q += 64) s = s + part[q];
      v[l] = s;
    }
    ifs_butterfly(v);
    tot = v[0];
  }
  return tot;
}
#endif

// L(η) at the interior cell c = (i, j) from η there (pc) and at its four neighbours (pw, pe, ps, pn)
__device__ inline double ifs_L(const IfsGeo& g, const IfsOp& o, int i, int j, double pc, double pw, double pe, double ps, double pn) {
  OCN_NO_CONTRACT
  const double dx = o.dxfc[j], rdx = o.r_dxfc[j];
  const double fe = o.Ax[(i + 1) + j * g.su] * hy_div(pe - pc, dx, rdx), fw = o.Ax[i + j * g.su] * hy_div(pc - pw, dx, rdx);
  const double fn = o.Ay[i + (j + 1) * g.sv] * hy_div(pn - pc, o.dycf[j + 1], o.r_dycf[j + 1]);
  const double fs = o.Ay[i + j * g.sv] * hy_div(pc - ps, o.dycf[j], o.r_dycf[j]);
  return ((fe - fw) + (fn - fs)) - hy_div(o.azcc[j] * pc, o.gdt2, o.r_gdt2);
}

// ---- the right-hand side and the first residual -------------------------------------------------------------------------------
// rhs = (δx ∫ᶻQ.u + δy ∫ᶻQ.v - Az η / Δt) / (g Δt), q = L(η) (η filled), r = b - q over the parent array, partials of r·r; resets
// the solver's scalars
__global__ void __launch_bounds__(IFS_NT) k_ifs_init(IfsGeo g, IfsOp o, const double* eta, const double* Qu, const double* Qv, double* rhs,
                                                     double* q, double* r, double* prr, IfsState* st, double dt, double gdt) {
  OCN_NO_CONTRACT
  if (blockIdx.x == 0 && threadIdx.x == 0) {
    st->it = 0; st->itA = 0; st->stop = 0; st->stopA = 0; st->nonfinite = 0;
    st->tol = 0.0; st->rnorm = 0.0; st->rho[0] = 0.0; st->rho[1] = 0.0;
  }
  const int n = g.Tx * g.Ty, stride = gridDim.x * IFS_NT;
  double acc = 0.0;
  for (int P = blockIdx.x * IFS_NT + threadIdx.x; P < n; P += stride) {
    const int j = P / g.Tx, i = P - j * g.Tx;
    if (i >= g.Hx && i < g.Hx + g.Nx && j >= g.Hy && j < g.Hy + g.Ny) {
      const double e = eta[P];
      const double dQ = (Qu[(i + 1) + j * g.su] - Qu[i + j * g.su]) + (Qv[i + (j + 1) * g.sv] - Qv[i + j * g.sv]);
      const double b = (dQ - o.azcc[j] * e / dt) / gdt;
      const double Lx = ifs_L(g, o, i, j, e, eta[P - 1], eta[P + 1], eta[P - g.Tx], eta[P + g.Tx]);
      rhs[P] = b;
      q[P] = Lx;
      const double rr = b - Lx;
      r[P] = rr;
      acc = acc + rr * rr;
    } else {
      r[P] = rhs[P] - q[P];
    }
  }
  ifs_block_partial(acc, prr);
}

// ---- iteration, first half: stop test, p, q = L(p), partials of p·q -------------------------------------------------------------
// pb[0], pb[1]: the two p buffers; iteration n reads pb[n & 1] and writes pb[(n + 1) & 1]
__global__ void __launch_bounds__(IFS_NT) k_ifs_pq(IfsGeo g, IfsOp o, const double* r, double* pb0, double* pb1, double* q, const double* prr,
                                                   double* ppq, IfsState* st, int nb, double reltol, double abstol, int maxiter) {
  OCN_NO_CONTRACT
  if (st->stop) return;
  const int it = st->it;
  const double rr = ifs_total(prr, nb);
  const double rnorm = sqrt(rr);
  const double tol = it == 0 ? fmax(reltol * rnorm, abstol) : st->tol;
  const bool lead = blockIdx.x == 0 && threadIdx.x == 0;
  const bool finite = rnorm <= 1.7976931348623157e308;           // false for inf and NaN
  if (it >= maxiter || rnorm <= tol || !finite) {                 // iterating(solver, tolerance), and a non-finite residual
    if (lead) {
      st->stopA = 1;
      st->rnorm = rnorm;
      st->nonfinite = !finite;
      if (it == 0) st->tol = tol;
    }
    return;
  }
  // z = r (no preconditioner); ρ = z·r
  const double rho = rr;
  const double beta = it == 0 ? 0.0 : rho / st->rho[(it - 1) & 1];
  if (lead) {
    st->itA = it;
    st->rho[it & 1] = rho;
    if (it == 0) st->tol = tol;
  }
  const double* po = (it & 1) ? pb1 : pb0;
  double* pn = (it & 1) ? pb0 : pb1;
  // p at a parent cell after the fill: the formed value at the cell the fill copies
  auto pat = [&](int i, int j) {
    const long s = ifs_src(g, i, j);
    return it == 0 ? r[s] : r[s] + beta * po[s];
  };
  const int n = g.Tx * g.Ty, stride = gridDim.x * IFS_NT;
  double acc = 0.0;
  for (int P = blockIdx.x * IFS_NT + threadIdx.x; P < n; P += stride) {
    const int j = P / g.Tx, i = P - j * g.Tx;
    const double pc = pat(i, j);
    pn[P] = pc;
    if (i >= g.Hx && i < g.Hx + g.Nx && j >= g.Hy && j < g.Hy + g.Ny) {
      const double Lp = ifs_L(g, o, i, j, pc, pat(i - 1, j), pat(i + 1, j), pat(i, j - 1), pat(i, j + 1));
      q[P] = Lp;
      acc = acc + pc * Lp;
    }
  }
  ifs_block_partial(acc, ppq);
}

// ---- iteration, second half: α, x += α p, r -= α q, partials of r·r ---------------------------------------------------------------
__global__ void __launch_bounds__(IFS_NT) k_ifs_xr(IfsGeo g, double* x, double* r, const double* pb0, const double* pb1, const double* q,
                                                   const double* ppq, double* prr, IfsState* st, int nb) {
  OCN_NO_CONTRACT
  if (st->stopA) {
    if (blockIdx.x == 0 && threadIdx.x == 0) st->stop = 1;
    return;
  }
  const int it = st->itA;
  const double pq = ifs_total(ppq, nb);
  const double alpha = st->rho[it & 1] / pq;
  const double* p = (it & 1) ? pb0 : pb1;
  const int n = g.Tx * g.Ty, stride = gridDim.x * IFS_NT;
  double acc = 0.0;
  for (int P = blockIdx.x * IFS_NT + threadIdx.x; P < n; P += stride) {
    const int j = P / g.Tx, i = P - j * g.Tx;
    x[P] = x[P] + alpha * p[P];
    const double rn = r[P] - alpha * q[P];
    r[P] = rn;
    if (i >= g.Hx && i < g.Hx + g.Nx && j >= g.Hy && j < g.Hy + g.Ny) acc = acc + rn * rn;
  }
  ifs_block_partial(acc, prr);
  if (blockIdx.x == 0 && threadIdx.x == 0) st->it = it + 1;
}

// ---- vertical integrals ---------------------------------------------------------------------------------------------------------
// sum!(∫ᶻQ.u, Ax * u): Q[i, j] = Σ_k (Δy[j] Δz[k]) u[i, j, k], level 1 first, over the field's interior (the boundary face of a Bounded
// direction included: the fill of Q zeroes it afterwards); arow: Δyᶠᶜ per row for u, Δxᶜᶠ for v
__global__ void k_ifs_vsum(double* Q, const double* u, const double* arow, const double* dzc, int Sx, int Sy, int Nz, int Hx, int Hy, int Hz,
                           long sy3, long sz3, long sy2) {
  OCN_NO_CONTRACT
  const int i = blockIdx.x * blockDim.x + threadIdx.x, j = blockIdx.y * blockDim.y + threadIdx.y;
  if (i >= Sx || j >= Sy) return;
  const double m = arow[j + Hy];
  long c = (i + Hx) + (long)(j + Hy) * sy3 + (long)Hz * sz3;
  double acc = 0.0;
  for (int k = 0; k < Nz; ++k, c += sz3) {
    const double q = (m * dzc[k]) * u[c];
    acc = k == 0 ? q : acc + q;
  }
  Q[(i + Hx) + (long)(j + Hy) * sy2] = acc;
}

// k_hy_momentum's pass for the implicit free surface: the AB2 step, the constant vertically implicit viscosity (forward elimination on the
// way up, back substitution on the way down) and G^- <- G^n, then sum!(∫ᶻQ, Ax * u) of the stepped column -- the same sum as
// k_ifs_vsum, without reading u again
__global__ void k_hy_momentum_ifs(double* u, const double* gn, double* gm, double* Q, const double* arow, double dt, double cn, double cm,
                                  const double* dzc, int Sx, int Sy, int Nx, int Ny, int Nz, int Hx, int Hy, int Hz, long sy3, long sz3, long sy2,
                                  HyImp imp, int implicit) {
  OCN_NO_CONTRACT
  const int i = blockIdx.x * blockDim.x + threadIdx.x, j = blockIdx.y * blockDim.y + threadIdx.y;
  if (i >= Sx || j >= Sy) return;
  const bool step = i < Nx && j < Ny;
  const double m = arow[j + Hy];
  const long c0 = (i + Hx) + (long)(j + Hy) * sy3 + (long)Hz * sz3;
  const bool imp_on = implicit && step;
  long c = c0;
  double a = 0.0, phi = 0.0;
  for (int k = 0; k < Nz; ++k, c += sz3) {
    const double uo = u[c];
    if (step) {
      const double n = gn[c];
      const double un = hy_ab2(uo, n, gm[c], dt, cn, cm);
      gm[c] = n;
      if (imp_on) {
        phi = k == 0 ? hy_div(un, imp.beta[0], imp.rbeta[0]) : hy_div(un - imp.a[k - 1] * phi, imp.beta[k], imp.rbeta[k]);
        u[c] = phi;
      } else {
        u[c] = un;
        const double q = (m * dzc[k]) * un;
        a = k == 0 ? q : a + q;
      }
    } else {
      const double q = (m * dzc[k]) * uo;
      a = k == 0 ? q : a + q;
    }
  }
  if (imp_on) {
    c = c0 + (long)(Nz - 1) * sz3;
    for (int k = Nz - 2; k >= 0; --k) {
      c -= sz3;
      phi = u[c] - imp.t[k + 1] * phi;
      u[c] = phi;
    }
    c = c0;
    for (int k = 0; k < Nz; ++k, c += sz3) {
      const double q = (m * dzc[k]) * u[c];
      a = k == 0 ? q : a + q;
    }
  }
  Q[(i + Hx) + (long)(j + Hy) * sy2] = a;
}

// ---- the barotropic pressure correction -----------------------------------------------------------------------------------------
// u[i, j, k] -= g Δt ∂xᶠᶜᶜ η, v[i, j, k] -= g Δt ∂yᶜᶠᶜ η over i = 1..Nx, j = 1..Ny, k = 1..Nz; one thread per column (the correction
// is that of every level).  eta points at the free surface's row that holds the grid's parent row 0 (a latitude band's rows).
__global__ void k_ifs_correct(double* u, double* v, const double* eta, const double* dxfc, const double* dycf, double gdt, int Nx, int Ny, int Nz,
                              int Hx, int Hy, int Hz, long su3, long szu, long sv3, long szv, long se) {
  OCN_NO_CONTRACT
  const int i = blockIdx.x * blockDim.x + threadIdx.x, j = blockIdx.y * blockDim.y + threadIdx.y;
  if (i >= Nx || j >= Ny) return;
  const int r = j + Hy;
  const long ce = (i + Hx) + (long)r * se;
  const double du = gdt * ((eta[ce] - eta[ce - 1]) / dxfc[r]), dv = gdt * ((eta[ce] - eta[ce - se]) / dycf[r]);
  long cu = (i + Hx) + (long)r * su3 + (long)Hz * szu, cv = (i + Hx) + (long)r * sv3 + (long)Hz * szv;
  for (int k = 0; k < Nz; ++k, cu += szu, cv += szv) {
    u[cu] = u[cu] - du;
    v[cv] = v[cv] - dv;
  }
}
