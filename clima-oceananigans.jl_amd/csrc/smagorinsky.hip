// smagorinsky.hip -- the eddy viscosity of SmagorinskyLilly (calculate_diffusivities!, smagorinsky_lilly.jl:99-124).
//
// Restated from the reference (paths relative to src/TurbulenceClosures of the reference unless noted):
//   turbulence_closure_implementations/smagorinsky_lilly.jl:68-69   C = 0.16, Cb = 1, Pr = 1
//   :85-88    stability function  s = 0 where Sigma^2 == 0, else sqrt(1 - min(1, Cb N^2 / Sigma^2))
//   :97-106   nu_e = s (C Delta_f)^2 sqrt(2 Sigma^2),  N^2 = max(0, I_z(d_z b)) from the faces k and k+1
//   :131      Delta_f = geo_mean (turbulence_closure_utils.jl:29-30): cbrt(dx dy dz_c(k))
//   :146-153  Sigma^2 at ccc = tr(Sigma^2) + 2 I_xy(Sigma_12^2) + 2 I_xz(Sigma_13^2) + 2 I_yz(Sigma_23^2): the strains are
//             squared where they live (ffc, fcf, cff; velocity_tracer_gradients.jl:25-46,78) and then averaged to the centre
//   ../BuoyancyModels/buoyancy_tracer.jl:16        d_z b = d_z(b)
//   ../BuoyancyModels/seawater_buoyancy.jl:171-176 d_z b = g (alpha d_z T - beta d_z S)   (LinearEquationOfState)
// kappa_e of a tracer is nu_e / Pr: never stored, the flux kernels read nu_e (kernels.hip k_tend_c, fused.hip k_tracer_step3)
// and form nu_e * (1 / Pr) with the reciprocal taken once on the host: a Pr that is no power of two gives the last bit of
// nu_e / Pr or its neighbour (one FP64 division per face and tracer saved; tests/test_smagorinsky_lilly.py ppb_pr_07).
//
// Two kernels write the interior of nu_e; the caller fills its halos.
//   k_smag_nu       tiled like k_rest4 (fused.hip): complete x rows in LDS, a march in z, every strain formed once
//   k_smag_nu_cell  one thread per cell, every configuration
#include "internal.h"

struct SmagArgs {
  const double *u, *v, *w;   // k_smag_nu: PARENT bases; k_smag_nu_cell: interior-origin pointers
  const double *q0, *q1;     // the buoyancy model's tracers, same convention: b (nb = 1), T and S (nb = 2)
  double* nu;
  const double* cd2;         // (C Delta_f)^2 of level k, entry [k]
  double Cb, cg, c0, c1;     // d_z b = d_z q0 (nb = 1) or cg (c0 d_z q0 - c1 d_z q1) (nb = 2)
  int nb;
  unsigned org;              // k_smag_nu: byte offset of the first interior cell in the parent
  int ntiles;
};

OCN_DEVFN double smag_sq(double x) { return x * x; }

// nu_e from Sigma^2, N^2 and (C Delta_f)^2 (smagorinsky_lilly.jl:85-88,97)
OCN_DEVFN double smag_nu(double S2, double N2, double Cb, double cd2) {
  if (S2 == 0.0) return 0.0;
  const double s = sqrt(1.0 - fmin(1.0, Cb * N2 / S2));
  return s * cd2 * sqrt(2.0 * S2);
}

// ---- one thread per cell ---------------------------------------------------------------------------------------------------
__global__ void k_smag_nu_cell(GridDev g, SmagArgs a) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  const int j = blockIdx.y * blockDim.y + threadIdx.y;
  const int k = blockIdx.z;   // one level per workgroup: the spacings are scalar loads
  if (i >= g.Nx || j >= g.Ny || k >= g.Nz) return;
  const long sy = g.sy, sz = g.sz;
  const long c = i + j * sy + k * sz;
  const double rdx = g.rdx, rdy = g.rdy;
  const double rf0 = g_rdzf(g, k), rf1 = g_rdzf(g, k + 1);
  const double *u = a.u, *v = a.v, *w = a.w;
  auto s12 = [&](long p) { return smag_sq(0.5 * ((u[p] - u[p - sy]) * rdy + (v[p] - v[p - 1]) * rdx)); };            // ffc
  auto s13 = [&](long p, double rf) { return smag_sq(0.5 * ((u[p] - u[p - sz]) * rf + (w[p] - w[p - 1]) * rdx)); };   // fcf
  auto s23 = [&](long p, double rf) { return smag_sq(0.5 * ((v[p] - v[p - sz]) * rf + (w[p] - w[p - sy]) * rdy)); };  // cff
  const double tr = smag_sq((u[c + 1] - u[c]) * rdx) + smag_sq((v[c + sy] - v[c]) * rdy) + smag_sq((w[c + sz] - w[c]) * g_rdzc(g, k));
  const double xy = 0.5 * (0.5 * (s12(c) + s12(c + 1)) + 0.5 * (s12(c + sy) + s12(c + 1 + sy)));
  const double xz = 0.5 * (0.5 * (s13(c, rf0) + s13(c + 1, rf0)) + 0.5 * (s13(c + sz, rf1) + s13(c + 1 + sz, rf1)));
  const double yz = 0.5 * (0.5 * (s23(c, rf0) + s23(c + sy, rf0)) + 0.5 * (s23(c + sz, rf1) + s23(c + sy + sz, rf1)));
  const double S2 = tr + 2.0 * xy + 2.0 * xz + 2.0 * yz;
  double N2 = 0.0;
  if (a.nb) {
    auto bz = [&](long p, double rf) {   // d_z b at the bottom face of cell p
      const double d0 = (a.q0[p] - a.q0[p - sz]) * rf;
      return a.nb == 2 ? a.cg * (a.c0 * d0 - a.c1 * ((a.q1[p] - a.q1[p - sz]) * rf)) : d0;
    };
    N2 = fmax(0.0, 0.5 * (bz(c, rf0) + bz(c + sz, rf1)));
  }
  a.nu[c] = smag_nu(S2, N2, a.Cb, a.cd2[k]);
}

// ---- tiled ---------------------------------------------------------------------------------------------------------------------
// The workgroup of k_rest4: BX x BY threads own the complete x rows j0 .. j0+BY-2 (+ one ghost row that only forms south-face
// values) and march over the levels of their segment; u, v, w of rows j0-1 .. j0+BY-1, columns -3 .. Nx+2, arrive by LDS DMA,
// double buffered.  At level k a thread forms, once, what lives at the WEST / SOUTH / BOTTOM edges of its cell --
// Sigma_12^2 at (x-face i, y-face j), Sigma_13^2 at (x-face i, z-face k), Sigma_23^2 at (y-face j, z-face k) -- plus
// Sigma_11^2 + Sigma_22^2 at the centre and d_z b at its bottom face (own column only: the buoyancy tracers are read straight
// from memory, one coalesced load per cell, and need no slab).  East values come by lane shift (wave-edge lanes: through LDS,
// one barrier later), north values through LDS, values at k+1 from the next level of the march.  One barrier per level, so the
// pipeline is three stages deep and nu_e of level k is written while level k+2 is in the slab:
//   step k    squares of level k; Sigma_12^2, Sigma_23^2 -> LDS (all lanes), Sigma_13^2 -> LDS (first lane of each wave)
//   step k+1  east / north values of level k are visible: I_xy(k), the x pair of Sigma_13^2(k), the y pair of Sigma_23^2(k);
//             w(k+1) completes tr(k), d_z b(k+1) completes N^2(k)
//   step k+2  the pairs of level k+1 complete I_xz(k) and I_yz(k): nu_e(k)
template <int BX, int BY>
__global__ void __launch_bounds__(BX* BY) k_smag_nu(GridDev g, SmagArgs a) {
  constexpr int T = BX * BY, NR = BY + 1, SX = BX + 6;      // rows j0-1 .. j0+BY-1; columns -3 .. Nx+2 (the parent row)
  constexpr int WV = BX < OCN_WAVE ? BX : OCN_WAVE, NW = BX / WV, NWV = T / WV;
  constexpr int SLAB = 3 * NR * SX;
  constexpr int NLDS = 2 * SLAB + 4 * T + 2 * BY * NW;
  static_assert(NLDS * sizeof(double) <= OCN_LDS_BYTES, "k_smag_nu: LDS footprint over 160 KiB (gfx950)");
  OCN_SHARED double lds[NLDS] __attribute__((aligned(16)));
  double* const fyb = lds + 2 * SLAB;    // [level parity][Sigma_12^2, Sigma_23^2][thread]
  double* const fxe = fyb + 4 * T;       // [level parity][row][wave]: Sigma_13^2 of the wave's first lane
  const int tx = threadIdx.x, ty = threadIdx.y;
  const int tid = ty * BX + tx;
  const int lane = tid % WV;
  const int wave = OCN_UNIFORM(tid / WV);
  const unsigned sxb = 8u, syb = (unsigned)g.sy * 8u, szb = (unsigned)g.sz * 8u;
  const double rdx = g.rdx, rdy = g.rdy;
  const bool ghost = (ty == BY - 1);
  const bool xedge = (tx % WV == WV - 1) || (tx + 1 >= g.Nx);
  const int txe = (tx + 1 >= g.Nx) ? 0 : tx + 1;
  const int tyn = ty + 1 < BY ? ty + 1 : ty;
  const int nid_e = ty * BX + txe, nid_n = tyn * BX + tx, nid_ne = tyn * BX + txe;
  const int eidx = ty * NW + txe / WV;
  const int nseg = gridDim.x, per = nseg / 8;
  const long seg = (nseg % 8 == 0) ? (long)(blockIdx.x % 8) * per + blockIdx.x / 8 : (long)blockIdx.x;
  const long total = (long)a.ntiles * g.Nz;
  long lo = seg * total / nseg;
  const long hi = (seg + 1) * total / nseg;
  const int PR = (g.Nx + 6) / 2;
  while (lo < hi) {
    const int tile = (int)(lo / g.Nz);
    const int k0 = (int)(lo - (long)tile * g.Nz);
    const int k1 = (k0 + (hi - lo) < g.Nz) ? (int)(k0 + (hi - lo)) : g.Nz;   // levels k0 .. k1-1 are written; level k1 supplies their top values
    lo += k1 - k0;
    const int j0 = tile * (BY - 1);
    const int j = j0 + ty;
    const bool ocol = tx < g.Nx;
    const bool do_y = ocol && j <= g.Ny;              // forms the south-face squares
    const bool full = ocol && j < g.Ny && !ghost;
    const unsigned cxy = a.org + (unsigned)(ocol ? tx : 0) * sxb + (unsigned)(j <= g.Ny ? j : 0) * syb;
    auto dma = [&](int k, int buf) {                  // rows j0-1 .. of level k, every field; wave w takes (field, row) pairs
      const long src0 = (long)a.org + ((long)(j0 - 1) * g.sy + (long)k * g.sz - 3) * 8;
      for (int fr = wave; fr < 3 * NR; fr += NWV) {
        const int f = fr / NR, r = fr - f * NR;
        const double* base = f == 0 ? a.u : f == 1 ? a.v : a.w;
        const unsigned so = (unsigned)(src0 + (long)r * g.sy * 8);
        char* dst = (char*)(lds + buf * SLAB + fr * SX);
        for (int q0 = 0; q0 < PR; q0 += WV)
          if (q0 + lane < PR) ocn_glds16((const char*)base + (so + 16u * (unsigned)(q0 + lane)), dst + 16 * q0, lane);
      }
    };
    // element (field f, row offset d in {-1, 0, +1}, column offset e) of the level's slab, relative to this thread's cell
#define RS(f, d, e) S[(f) * NR * SX + ((d) + 1) * SX + (e) + 3]
    // carried from the level below: own u, v and the buoyancy tracers
    const unsigned cb = cxy + (unsigned)k0 * szb - szb;
    double up = ldo(a.u, cb), vp = ldo(a.v, cb);
    double q0p = a.nb ? ldo(a.q0, cb) : 0.0, q1p = a.nb == 2 ? ldo(a.q1, cb) : 0.0;
    // stage 1 -> 2 (level k-1 at step k): own squares, lane-shifted east values, centre part, d_z b, w
    double s12 = 0, s13 = 0, s23 = 0, e12 = 0, e13 = 0, h12 = 0, bzp = 0, wp = 0;
    // stage 2 -> 3 (level k-2 at step k)
    double tr2 = 0, xy2 = 0, x13 = 0, y23 = 0, n2 = 0;
    __syncthreads();
    dma(k0, 0);
    for (int k = k0; k <= k1 + 1; ++k) {
      const int kb = (k - k0) & 1;
      const bool slab = (k <= k1);                    // level k is in the slab; k1 + 1: drain
      __syncthreads();
      if (k < k1) dma(k + 1, kb ^ 1);
      const double* S = lds + kb * SLAB + ty * SX + tx;
      const unsigned c = cxy + (unsigned)k * szb;
      double uc = 0, vc = 0, wc = 0, bz = 0, q0c = 0, q1c = 0;
      if (slab) {
        uc = RS(0, 0, 0); vc = RS(1, 0, 0); wc = RS(2, 0, 0);
        if (a.nb && full) {
          const double rzf = g_rdzf(g, k);
          q0c = ldo(a.q0, c);
          bz = (q0c - q0p) * rzf;
          if (a.nb == 2) {
            q1c = ldo(a.q1, c);
            bz = a.cg * (a.c0 * bz - a.c1 * ((q1c - q1p) * rzf));
          }
        }
      }
      if (k > k0) {
        // level k-1: the neighbours' squares, written before the barrier above
        const double* fyp = fyb + (kb ^ 1) * 2 * T;
        const double e12v = xedge ? fyp[nid_e] : e12;
        const double e13v = xedge ? fxe[(kb ^ 1) * BY * NW + eidx] : e13;
        const double xy1 = 0.5 * (0.5 * (s12 + e12v) + 0.5 * (fyp[nid_n] + fyp[nid_ne]));
        const double x13n = 0.5 * (s13 + e13v);
        const double y23n = 0.5 * (s23 + fyp[T + nid_n]);
        if (k >= k0 + 2 && full) {                    // level k-2 is complete
          const double S2 = tr2 + 2.0 * xy2 + 2.0 * (0.5 * (x13 + x13n)) + 2.0 * (0.5 * (y23 + y23n));
          *(double*)((char*)a.nu + (c - 2u * szb)) = smag_nu(S2, n2, a.Cb, a.cd2[k - 2]);
        }
        xy2 = xy1; x13 = x13n; y23 = y23n;
        tr2 = h12 + smag_sq((wc - wp) * g_rdzc(g, k - 1));   // used only when level k-1 is written (k <= k1: w of level k is there)
        n2 = fmax(0.0, 0.5 * (bzp + bz));
      }
      if (slab) {
        const double rzf = g_rdzf(g, k);
        s12 = smag_sq(0.5 * ((uc - RS(0, -1, 0)) * rdy + (vc - RS(1, 0, -1)) * rdx));    // (x-face i, y-face j)
        s13 = smag_sq(0.5 * ((uc - up) * rzf + (wc - RS(2, 0, -1)) * rdx));              // (x-face i, z-face k)
        s23 = smag_sq(0.5 * ((vc - vp) * rzf + (wc - RS(2, -1, 0)) * rdy));              // (y-face j, z-face k)
        h12 = full ? smag_sq((RS(0, 0, 1) - uc) * rdx) + smag_sq((RS(1, 1, 0) - vc) * rdy) : 0.0;   // centre: Sigma_11^2 + Sigma_22^2
        if (do_y) {
          double* fyn = fyb + kb * 2 * T;
          fyn[tid] = s12;
          fyn[T + tid] = s23;
        }
        e12 = ocn_shfl_next(s12);
        e13 = ocn_shfl_next(s13);
        if (tx % WV == 0 && do_y) fxe[kb * BY * NW + ty * NW + tx / WV] = s13;
        up = uc; vp = vc; wp = wc; bzp = bz; q0p = q0c; q1p = q1c;
      }
    }
#undef RS
  }
}

// per-level (C Delta_f)^2 with Delta_f = cbrt(dx dy dz_c(k)) (smagorinsky_lilly.jl:131, turbulence_closure_utils.jl:29-30)
int smag_build_table(ocn_model* m) {
  const ocn_grid* g = m->g;
  const GridDev& gd = m->gd;
  std::vector<double> t((size_t)gd.Nz);
  for (int k = 0; k < gd.Nz; ++k) {
    const double dzc = g->z_regular ? gd.dz : g->h_dzc[k + gd.Hz];
    const double cd = m->smag_C * std::cbrt(gd.dx * gd.dy * dzc);
    t[k] = cd * cd;
  }
  if (hipMalloc((void**)&m->smag_tab, t.size() * sizeof(double)) != hipSuccess) return OCN_ENOMEM;
  if (hipMemcpy(m->smag_tab, t.data(), t.size() * sizeof(double), hipMemcpyHostToDevice) != hipSuccess) {
    hipFree(m->smag_tab);
    m->smag_tab = nullptr;
    return OCN_EHIP;
  }
  return OCN_OK;
}

// k_smag_nu shares k_rest4's slab layout: exactly where that kernel serves the model (whole rows up to 256 columns, no wall
// in x, H = 3, the LDS-DMA row layout, the tiled "rest" path on: Bounded z, or Periodic regular z), on one rank
bool smag_tiled_ok(const ocn_model* m) {
  return m->d.closure == OCN_CLOSURE_SMAG && rest4_ok(m) && !m->g->dist && !m->g->dist_y && !m->knob_no_smag_tiled;
}

void launch_smag(ocn_model* m) {
  ProfScope ps(m->ctx, "smagorinsky_diffusivities");
  const GridDev& gd = m->gd;
  hipStream_t s = m->ctx->stream;
  const bool tiled = smag_tiled_ok(m);
  SmagArgs a;
  memset(&a, 0, sizeof(a));
  auto ptr = [&](Field& f) { return tiled ? f.d : f.interior(); };
  a.u = ptr(m->u); a.v = ptr(m->v); a.w = ptr(m->w);
  a.nu = ptr(m->nu_e);
  a.cd2 = m->smag_tab;
  a.Cb = m->smag_Cb;
  if (m->d.buoyancy == OCN_BUOYANCY_TRACER) {
    a.nb = 1;
    a.q0 = ptr(m->tr[m->d.b_index]);
  } else if (m->d.buoyancy == OCN_BUOYANCY_LINEAR_TS) {
    a.nb = 2;
    a.q0 = ptr(m->tr[m->d.T_index]);
    a.q1 = ptr(m->tr[m->d.S_index]);
    a.cg = m->d.g; a.c0 = m->d.alpha; a.c1 = m->d.beta;
  }
  if (!tiled) {
    const dim3 b(64, 4, 1), gr((gd.Nx + b.x - 1) / b.x, (gd.Ny + b.y - 1) / b.y, gd.Nz);
    ocn_launch(k_smag_nu_cell, gr, b, s, gd, a);
    return;
  }
  a.org = (unsigned)((m->u.Hx + m->u.Hy * m->u.sy + m->u.Hz * m->u.sz) * sizeof(double));
  int bx = gd.Nx <= 64 ? 64 : gd.Nx <= 128 ? 128 : 256;
  int by = bx == 256 ? 4 : 8;
#ifdef OCN_HOST_EMU
  if (gd.Nx <= 16) {   // the emulation runs one OS thread per GPU thread
    bx = 16;
    by = 4;
  }
#endif
  a.ntiles = (gd.Ny + by - 2) / (by - 1);
  int nseg = fused_cu_count(m);                   // one equal segment of the (tile, level) space per CU
  const long total = (long)a.ntiles * gd.Nz;
  if (nseg > total / 4) nseg = (int)(total / 4 > 8 ? total / 4 : 8);
  nseg = ((nseg + 7) / 8) * 8;                    // the XCD-aware remap inside the kernel wants a multiple of 8
#ifdef OCN_HOST_EMU
  nseg = total >= 3 ? 3 : 1;
#endif
  const dim3 blk(bx, by, 1), grd(nseg, 1, 1);
#ifdef OCN_HOST_EMU
  if (bx == 16) ocn_launch_sync(k_smag_nu<16, 4>, grd, blk, s, gd, a); else
#endif
  if (bx == 256) ocn_launch_sync(k_smag_nu<256, 4>, grd, blk, s, gd, a);
  else if (bx == 128) ocn_launch_sync(k_smag_nu<128, 8>, grd, blk, s, gd, a);
  else ocn_launch_sync(k_smag_nu<64, 8>, grd, blk, s, gd, a);
}
