// hyflux.h -- the flux boundary conditions of the HydrostaticFreeSurfaceModel, included by splitexplicit.hip after HyMetric (it shares
// that file's metric tables and its no-contraction rule).
//
//   reference (paths relative to the reference's src/)                                          here
//   Models/HydrostaticFreeSurfaceModels/calculate_hydrostatic_free_surface_tendencies.jl:205-240   hydro_flux_bcs (splitexplicit.hip)
//     calculate_hydrostatic_boundary_tendency_contributions!: apply_flux_bcs! of u, v and every tracer after the interior kernels
//   BoundaryConditions/apply_flux_bcs.jl:79-160 (apply_{x,y,z}_{west,...,top}_bc!)              k_hy_flux_x, k_hy_flux_y, k_hy_flux_z
//   BoundaryConditions/boundary_condition.jl:106-113 (getbc: a Number, an array, Nothing)        HyFluxBC::kind 1, 2 (0: no entry)
//   Operators/spacings_and_areas_and_volumes.jl:172-240 (Ax = Dy Dz, Ay = Dx Dz, Az, V = Az Dz)
//
// West / south / bottom: G[1] += (getbc * A(first face)) / V(first cell); east / north / top: G[N] -= (getbc * A(N + 1)) / V(N),
// the reference's operand order, IEEE division, no contraction.  Kind 3 is the discrete-form condition of the forced validation
// scripts (linear drag): getbc = -r * f[i, j, k_b] with f the field itself at its boundary level.  Regular longitude / rectilinear
// metrics: Az^fc = Az^cc, Az^cf = Az^ff, Dx^ff = Dx^cf, Dy^ff = Dy^cf, so every area is a row of the tables HyMetric carries.
//
// The reference launches x, then y, then z (apply_flux_bcs!), and each of its kernels applies the low side before the high one; a
// cell in a corner receives its terms in that order here too: one launch per direction, in that order, and the descriptors of a
// field are sorted by side.  Each launch carries every active condition of every field in one table (HyFluxTab, kernel arguments),
// so a thread reads each needed array once and read-modify-writes each needed G value once.  The table is indexed with constants
// only (the loop is unrolled), so it stays in scalar registers and the kernels hold no scratch.
//
// Latitude bands: arrays are per band (the mirror slices the global rows); x sides take the band's rows; south / north conditions
// are only put in the table of the band that touches that wall.
constexpr int HY_FLUX_MAX = 16;

struct HyFluxBC {
  double* G;             // G^n, parent array
  const double* f;       // kind 3: the field itself (same location and parent shape as G)
  const double* a;       // kind 2: the condition, first index fastest (z: Nx x Ny, x: Ny x Nz, y: Nx x Nz of this grid or band)
  double value;          // kind 1: the flux; kind 3: the rate r >= 0
  long sy, sz;           // parent strides of G and f
  int kind, side, loc;   // kind 1..3; side OCN_WEST .. OCN_TOP; loc 0 (Center, Center), 1 (Face, Center): u, 2 (Center, Face): v
};

struct HyFluxTab {
  HyFluxBC e[HY_FLUX_MAX];
  int n;
};

// z sides: one thread per column (i, j), 64-wide rows of threads (the per-row metrics are wave-uniform), consecutive i in consecutive
// lanes: every array, field and G access is a coalesced row access
__global__ void __launch_bounds__(256) k_hy_flux_z(HyMetric g, HyFluxTab t) {
  OCN_NO_CONTRACT
  const int i = blockIdx.x * blockDim.x + threadIdx.x, j = blockIdx.y * blockDim.y + threadIdx.y;
  if (i >= g.Nx || j >= g.Ny) return;
  const int r = OCN_UNIFORM(j + g.Hy);       // blockDim.x == 64: one row per wave
  const double azcc = g.azcc[r], azff = g.azff[r], dzb = g.dzc[0], dzt = g.dzc[g.Nz - 1];
  const long cell = (long)i + (long)j * g.Nx;
#pragma unroll
  for (int q = 0; q < HY_FLUX_MAX; ++q) {
    if (q >= t.n) continue;          // uniform; constant indices keep the table in scalar registers
    const HyFluxBC& e = t.e[q];
    const bool top = e.side == OCN_TOP;
    const long c = (i + g.Hx) + (long)r * e.sy + (long)((top ? g.Nz - 1 : 0) + g.Hz) * e.sz;
    const double F = e.kind == 1 ? e.value : e.kind == 2 ? e.a[cell] : (-e.value) * e.f[c];
    const double Az = e.loc == 2 ? azff : azcc;                       // Az^cf = Az^ff; Az^fc = Az^cc
    const double d = (F * Az) / (Az * (top ? dzt : dzb));
    e.G[c] = top ? e.G[c] - d : e.G[c] + d;
  }
}

// x sides: one thread per (j, k) of the grid or band; tracers (Ax^fcc = Dy^fc Dz, V^ccc) and v on a Bounded x (Ax^ffc = Dy^ff Dz, V^cfc)
__global__ void __launch_bounds__(256) k_hy_flux_x(HyMetric g, HyFluxTab t) {
  OCN_NO_CONTRACT
  const int j = blockIdx.x * blockDim.x + threadIdx.x, k = blockIdx.y;
  if (j >= g.Ny) return;
  const int r = j + g.Hy;
  const double dz = g.dzc[k];
  const long cell = (long)j + (long)k * g.Ny;
#pragma unroll
  for (int q = 0; q < HY_FLUX_MAX; ++q) {
    if (q >= t.n) continue;          // uniform; constant indices keep the table in scalar registers
    const HyFluxBC& e = t.e[q];
    const bool east = e.side == OCN_EAST;
    const long c = ((east ? g.Nx - 1 : 0) + g.Hx) + (long)r * e.sy + (long)(k + g.Hz) * e.sz;
    const double F = e.kind == 1 ? e.value : e.a[cell];
    const double A = (e.loc == 2 ? g.dycf[r] : g.dyfc[r]) * dz, V = (e.loc == 2 ? g.azff[r] : g.azcc[r]) * dz;
    const double d = (F * A) / V;
    e.G[c] = east ? e.G[c] - d : e.G[c] + d;
  }
}

// y sides: one thread per (i, k) at the first / last row of the grid (of a band touching that wall); tracers (Ay^cfc = Dx^cf Dz at
// the face row, V^ccc) and u on a Bounded y (Ay^ffc = Dx^ff Dz, V^fcc)
__global__ void __launch_bounds__(256) k_hy_flux_y(HyMetric g, HyFluxTab t) {
  OCN_NO_CONTRACT
  const int i = blockIdx.x * blockDim.x + threadIdx.x, k = blockIdx.y;
  if (i >= g.Nx) return;
  const double dz = g.dzc[k];
  const long cell = (long)i + (long)k * g.Nx;
#pragma unroll
  for (int q = 0; q < HY_FLUX_MAX; ++q) {
    if (q >= t.n) continue;          // uniform; constant indices keep the table in scalar registers
    const HyFluxBC& e = t.e[q];
    const bool north = e.side == OCN_NORTH;
    const int r = (north ? g.Ny - 1 : 0) + g.Hy;                       // the boundary cell's row; its outer face: r + 1 (north), r (south)
    const long c = (i + g.Hx) + (long)r * e.sy + (long)(k + g.Hz) * e.sz;
    const double F = e.kind == 1 ? e.value : e.a[cell];
    const double A = g.dxcf[north ? r + 1 : r] * dz, V = g.azcc[r] * dz;   // Dx^ff = Dx^cf; Az^fc = Az^cc
    const double d = (F * A) / V;
    e.G[c] = north ? e.G[c] - d : e.G[c] + d;
  }
}
