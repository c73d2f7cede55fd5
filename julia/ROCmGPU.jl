# ROCmGPU.jl -- the shim a maintainer adds to Oceananigans to route the NonhydrostaticModel hot path to
# libocnhip.so.  NOT executed in this repository (no Julia toolchain in the build image); it documents the
# reference-side binding of every entry point of include/ocnhip.h.
#
# Strategy (SURVEY.md section 8b): `ROCmGPU <: AbstractArchitecture` owns a context; the *model* is mirrored
# by an `ocn_model` handle whose device arrays are aliased by the Julia `Field`s (same parent layout), and
# the phase-level functions are overloaded so that no KernelAbstractions kernel is ever launched.

module ROCmGPUShim

using Oceananigans
using Oceananigans.Architectures: AbstractArchitecture
using OffsetArrays
import Oceananigans.Architectures: device, array_type, arch_array, device_event, architecture
import Oceananigans.TimeSteppers: time_step!, ab2_step!, rk3_substep!, store_tendencies!, update_state!,
                                  calculate_tendencies!, calculate_pressure_correction!, pressure_correct_velocities!
import Oceananigans.BoundaryConditions: fill_halo_regions!
import Oceananigans.Fields: set!

const libocnhip = get(ENV, "OCNHIP_LIB", "libocnhip.so")

check(rc, ctx=C_NULL) = rc == 0 ? nothing :
    error("libocnhip: ", unsafe_string(ccall((:ocn_last_error, libocnhip), Cstring, (Ptr{Cvoid},), ctx)))

# ---- architecture (src/Architectures.jl:53-142) ---------------------------------------------------------
mutable struct ROCmGPU <: AbstractArchitecture
    ctx :: Ptr{Cvoid}
end

function ROCmGPU(device_id::Integer = 0)
    ctx = Ref{Ptr{Cvoid}}(C_NULL)
    check(ccall((:ocn_init, libocnhip), Cint, (Cint, Ref{Ptr{Cvoid}}), device_id, ctx))
    arch = ROCmGPU(ctx[])
    finalizer(a -> ccall((:ocn_destroy, libocnhip), Cvoid, (Ptr{Cvoid},), a.ctx), arch)
    return arch
end

# A device array = library-owned memory + the parent size; host copies go through upload / download.
struct ROCArray{T, N} <: AbstractArray{T, N}
    ptr  :: Ptr{T}
    dims :: NTuple{N, Int}
end
Base.size(a::ROCArray) = a.dims
array_type(::ROCmGPU) = ROCArray
device_event(::ROCmGPU) = nothing                     # one in-order stream replaces KA events
Base.wait(::ROCmGPU, ::Nothing) = nothing

# ---- grid + model handles ----------------------------------------------------------------------------------
struct GridDesc                                        # mirrors `ocn_grid_desc` field by field
    N::NTuple{3, Int32}; H::NTuple{3, Int32}; topology::NTuple{3, Int32}
    x0::NTuple{3, Float64}; L::NTuple{3, Float64}; z_faces::Ptr{Float64}; rank::Int32; nranks::Int32
end

topo_code(::Type{Periodic}) = Int32(0); topo_code(::Type{Bounded}) = Int32(1); topo_code(::Type{Flat}) = Int32(2)

function ocn_grid(arch::ROCmGPU, grid::RectilinearGrid)
    TX, TY, TZ = topology(grid)
    zf = grid.Δzᵃᵃᶜ isa Number ? C_NULL : pointer(collect(Float64, grid.zᵃᵃᶠ[1:grid.Nz+1]))
    desc = GridDesc((grid.Nx, grid.Ny, grid.Nz), (grid.Hx, grid.Hy, grid.Hz), topo_code.((TX, TY, TZ)),
                    (grid.xᶠᵃᵃ[1], grid.yᵃᶠᵃ[1], grid.zᵃᵃᶠ[1]), (grid.Lx, grid.Ly, grid.Lz), zf, 0, 1)
    h = Ref{Ptr{Cvoid}}(C_NULL)
    check(ccall((:ocn_grid_create, libocnhip), Cint, (Ptr{Cvoid}, Ref{GridDesc}, Ref{Ptr{Cvoid}}), arch.ctx, desc, h), arch.ctx)
    return h[]
end

# `ocn_model_desc` (include/ocnhip.h; OCN_ABI_VERSION 5), field by field.  isbits, so it crosses ccall by reference.
const MAXTR = 8
struct BC; kind::Int32; value::Float64; array::Ptr{Float64}; end                       # ocn_bc
struct ModelDesc
    advection::Int32; stepper::Int32; chi::Float64; n_tracers::Int32; closure::Int32
    nu::Float64; kappa::NTuple{MAXTR, Float64}
    amd_Cnu::Float64; amd_Ckappa::NTuple{MAXTR, Float64}; amd_Cb::Float64; amd_has_Cb::Int32
    coriolis_fplane::Int32; f::Float64
    buoyancy::Int32; b_index::Int32; T_index::Int32; S_index::Int32; g::Float64; alpha::Float64; beta::Float64
    bcs::NTuple{3 + MAXTR, NTuple{6, BC}}                                               # [u, v, w, tracers...][west .. top]
    nu_bcs::NTuple{6, BC}; kappa_bcs::NTuple{MAXTR, NTuple{6, BC}}                      # AMD diffusivity fields (model.diffusivity_fields)
end

adv_code(::Nothing) = Int32(0); adv_code(::CenteredSecondOrder) = Int32(1); adv_code(::CenteredFourthOrder) = Int32(2)
adv_code(::UpwindBiasedFifthOrder) = Int32(3); adv_code(a::WENO5) = a isa WENO5{<:Any, <:Any, <:Any, <:Any, <:Any, true} ? Int32(4) : Int32(5)  # zweno / JS
adv_code(::UpwindBiasedFirstOrder) = Int32(6); adv_code(::UpwindBiasedThirdOrder) = Int32(7)

# one side of one field: BoundaryCondition{Flux | Value | Gradient | Open | Periodic, Nothing | Number | Array}
function bc_of(bc, keep)
    cls = bc.classification
    kind = cls isa Periodic ? 1 : cls isa Flux ? (bc.condition === nothing ? 2 : 3) : cls isa Value ? 4 : cls isa Gradient ? 5 :
           cls isa Open ? 6 : 0
    c = bc.condition
    c isa Function && error("function boundary conditions cannot cross the C ABI")     # ContinuousBoundaryFunction etc.
    c isa AbstractArray && (a = collect(Float64, c); push!(keep, a); return BC(kind, 0.0, pointer(a)))
    return BC(kind, c === nothing ? 0.0 : Float64(c), C_NULL)
end

# `ocn_tilted_desc` (include/ocnhip.h), field by field: Buoyancy{M, <:Tuple} and ConstantCartesianCoriolis map onto it.  The drag
# slots ([u, v][bottom, top]: present, cd, u_background, v_background) stay empty here: the reference writes its drag as a
# ContinuousBoundaryFunction, which cannot cross the C ABI (bc_of refuses it); the library offers it by parameters.
struct QuadraticDrag; present::Int32; cd::Float64; u_background::Float64; v_background::Float64; end
struct TiltedDesc
    has_gravity_vector::Int32; gx::Float64; gy::Float64; gz::Float64
    coriolis_cartesian::Int32; fx::Float64; fy::Float64; fz::Float64
    drag::NTuple{2, NTuple{2, QuadraticDrag}}
end
function tilted_desc(m)
    nodrag = ntuple(_ -> ntuple(_ -> QuadraticDrag(0, 0.0, 0.0, 0.0), 2), 2)
    ĝ = m.buoyancy === nothing ? nothing : m.buoyancy.gravity_unit_vector
    g = ĝ isa Tuple ? (Int32(1), Float64.(ĝ)...) : (Int32(0), 0.0, 0.0, 0.0)              # ZDirection: the plain kernels
    c = m.coriolis
    f = c isa ConstantCartesianCoriolis ? (Int32(1), Float64(c.fx), Float64(c.fy), Float64(c.fz)) : (Int32(0), 0.0, 0.0, 0.0)
    return TiltedDesc(g..., f..., nodrag)
end

function ocn_model(arch::ROCmGPU, gridh, m)                                             # m: the fields NonhydrostaticModel(...) assembled
    bplan = background_plan(m)                                                          # which members exist and in which form
    fplan = forcing_plan(m)                                                             # refuses what cannot be tabulated, by name
    m.stokes_drift === nothing || m.stokes_drift isa UniformStokesDrift || error("stokes_drift: only UniformStokesDrift is on the path")
    names = keys(m.tracers); nt = length(names)
    pad(t) = ntuple(i -> i <= length(t) ? Float64(t[i]) : 0.0, MAXTR)
    cl = m.closure
    closure, nu, kap, Cnu, Ck, Cb, hasCb = Int32(0), 0.0, pad(()), 0.0, pad(()), 0.0, Int32(0)
    if cl isa ScalarDiffusivity
        closure, nu, kap = Int32(1), cl.ν, pad(values(cl.κ))
    elseif cl isa AnisotropicMinimumDissipation
        closure, Cnu, Ck = Int32(2), cl.Cν, pad(values(cl.Cκ))
        cl.Cb === nothing || ((Cb, hasCb) = (Float64(cl.Cb), Int32(1)))
    elseif cl !== nothing
        error("closure $(typeof(cl)) is outside the path")
    end
    idx(n) = Int32(something(findfirst(==(n), names), 0) - 1)
    b = m.buoyancy === nothing ? nothing : m.buoyancy.model
    buoy, g, α, β = b === nothing ? (Int32(0), 0.0, 0.0, 0.0) : b isa BuoyancyTracer ? (Int32(1), 0.0, 0.0, 0.0) :
                    (Int32(2), b.gravitational_acceleration, b.equation_of_state.thermal_expansion, b.equation_of_state.haline_contraction)
    keep = Any[]                                                                        # host arrays stay alive across the call
    sides(f) = (bcs = f.boundary_conditions; ntuple(s -> bc_of((bcs.west, bcs.east, bcs.south, bcs.north, bcs.bottom, bcs.top)[s], keep), 6))
    none = ntuple(_ -> BC(0, 0.0, C_NULL), 6)
    fields = (m.velocities.u, m.velocities.v, m.velocities.w, values(m.tracers)...)
    desc = ModelDesc(adv_code(m.advection), m.timestepper isa RungeKutta3TimeStepper ? 1 : 0,
                     m.timestepper isa QuasiAdamsBashforth2TimeStepper ? m.timestepper.χ : 0.1, nt, closure, nu, kap, Cnu, Ck, Cb, hasCb,
                     m.coriolis isa FPlane ? 1 : 0, m.coriolis isa FPlane ? m.coriolis.f : 0.0,       # ConstantCartesianCoriolis: tilted_desc
                     buoy, idx(:b), idx(:T), idx(:S), g, α, β,
                     ntuple(i -> i <= length(fields) ? sides(fields[i]) : none, 3 + MAXTR),
                     closure == 2 ? sides(m.diffusivity_fields.νₑ) : none,
                     ntuple(i -> (closure == 2 && i <= nt) ? sides(m.diffusivity_fields.κₑ[i]) : none, MAXTR))
    h = Ref{Ptr{Cvoid}}(C_NULL)
    m.coriolis === nothing || m.coriolis isa FPlane || m.coriolis isa ConstantCartesianCoriolis || error("coriolis $(typeof(m.coriolis)) is outside the path")
    td = tilted_desc(m)
    if td.has_gravity_vector != 0 || td.coriolis_cartesian != 0   # a gravity unit vector or a Cartesian rotation: the general creator; forcing and background ride along
        fd = UInt32[fplan.column_fields, fplan.field_fields]; bd = UInt32[bplan.column_members, bplan.field_members]
        GC.@preserve keep fd bd check(ccall((:ocn_model_create_tilted, libocnhip), Cint,
                                            (Ptr{Cvoid}, Ref{ModelDesc}, Ptr{Cvoid}, UInt32, Ptr{UInt32}, Ptr{UInt32}, Ref{TiltedDesc}, Ref{Ptr{Cvoid}}),
                                            gridh, desc, C_NULL, UInt32(m.stokes_drift === nothing ? 0 : 1), fd, bd, td, h), arch.ctx)
    elseif bplan.column_members | bplan.field_members != 0   # background fields: ocn_background_desc { column_members, field_members }; forcing rides along
        fd = UInt32[fplan.column_fields, fplan.field_fields]; bd = UInt32[bplan.column_members, bplan.field_members]
        GC.@preserve keep fd bd check(ccall((:ocn_model_create_background, libocnhip), Cint,
                                            (Ptr{Cvoid}, Ref{ModelDesc}, Ptr{Cvoid}, UInt32, Ptr{UInt32}, Ptr{UInt32}, Ref{Ptr{Cvoid}}),
                                            gridh, desc, C_NULL, UInt32(m.stokes_drift === nothing ? 0 : 1), fd, bd, h), arch.ctx)
    elseif fplan.column_fields | fplan.field_fields != 0   # forcing is a creation-time property too: ocn_forcing_desc { column_fields, field_fields }
        fd = UInt32[fplan.column_fields, fplan.field_fields]
        GC.@preserve keep fd check(ccall((:ocn_model_create_forced, libocnhip), Cint,
                                         (Ptr{Cvoid}, Ref{ModelDesc}, Ptr{Cvoid}, UInt32, Ptr{UInt32}, Ref{Ptr{Cvoid}}),
                                         gridh, desc, C_NULL, UInt32(m.stokes_drift === nothing ? 0 : 1), fd, h), arch.ctx)
    elseif m.stokes_drift === nothing
        GC.@preserve keep check(ccall((:ocn_model_create, libocnhip), Cint, (Ptr{Cvoid}, Ref{ModelDesc}, Ref{Ptr{Cvoid}}), gridh, desc, h), arch.ctx)
    else  # a creation-time property: it decides the kernels.  OCN_FEATURE_STOKES_DRIFT = 1; a SmagorinskyLilly desc goes where C_NULL is
        GC.@preserve keep check(ccall((:ocn_model_create_with, libocnhip), Cint, (Ptr{Cvoid}, Ref{ModelDesc}, Ptr{Cvoid}, UInt32, Ref{Ptr{Cvoid}}),
                                      gridh, desc, C_NULL, UInt32(1), h), arch.ctx)
    end
    return h[]
end

# Stand-alone fields -- Field{LX, LY, LZ}(grid), CenterField(grid), zeros(FT, ::ROCmGPU, N...) (Fields/field.jl:16-30,
# Grids/zeros.jl:7): ocn_field_create gives a zero-filled parent array with the layout of the model's own fields.
loc_code(::Type{Center}) = Int32(0); loc_code(::Type{Face}) = Int32(1)
function new_field_data(gridh, grid, loc, ctx)
    h = Ref{Ptr{Cvoid}}(C_NULL)
    check(ccall((:ocn_field_create, libocnhip), Cint, (Ptr{Cvoid}, Cint, Cint, Cint, Ref{Ptr{Cvoid}}), gridh, loc_code.(loc)..., h), ctx)
    p = ccall((:ocn_field_parent_ptr, libocnhip), Ptr{Float64}, (Ptr{Cvoid},), h[])
    T = Oceananigans.Grids.total_size(loc, grid)      # dense on (Periodic, Periodic, *) grids; ocn_field_parent_layout otherwise, as in alias_field_data
    return Oceananigans.Grids.offset_data(unsafe_wrap(ROCArray, p, T), grid, loc), h[]   # keep h: ocn_field_destroy in the finalizer
end

# Field data alias the library's parent arrays (same layout as Grids/new_data.jl:33-61).  With walls or slices in
# x / y the allocation is pitched: ocn_field_layout gives element strides and the origin of the logical parent.
# u, v, w, both pressures, nu_e and kappa_e keep their device pointers for the life of the model (alias once, at model
# construction); G^n / G^- and, on the tiled kernels' paths, the tracers are double buffered: call this again after every
# time_step! for those fields (include/ocnhip.h, "pointer stability"; tests/test_model_contracts.py).
function alias_field_data(model_handle, field_id, grid, loc)
    p = ccall((:ocn_field_device_ptr, libocnhip), Ptr{Float64}, (Ptr{Cvoid}, Cint), model_handle, field_id)
    st = zeros(Int64, 3); org = Ref(Int64(0))
    ccall((:ocn_field_layout, libocnhip), Cint, (Ptr{Cvoid}, Cint, Ptr{Int64}, Ref{Int64}), model_handle, field_id, st, org)
    T = Oceananigans.Grids.total_size(loc, grid)
    Px, Py = st[2], st[3] ÷ st[2]
    whole = unsafe_wrap(ROCArray, p, (Px, Py, T[3]))
    ox, oy = org[] % Px, org[] ÷ Px
    parent = (Px, Py) == T[1:2] ? whole : view(whole, ox .+ (1:T[1]), oy .+ (1:T[2]), :)
    return Oceananigans.Grids.offset_data(parent, grid, loc)
end

# ---- phase-level overloads (each is ONE ccall) ---------------------------------------------------------------
const RM = NonhydrostaticModel{<:Any, <:Any, <:ROCmGPU}   # models living on ROCmGPU (handle kept in model.auxiliary_fields.ocn)
handle(m) = m.auxiliary_fields.ocn

# stokes_drift = UniformStokesDrift(∂z_uˢ, ∂z_vˢ, ∂t_uˢ, ∂t_vˢ) (StokesDrift.jl:46-80): the four functions of (z, t) stay in Julia and
# are evaluated into six tables of Nz numbers per stage -- at znode(Center, k) and znode(Face, k), k = 1..Nz, and at the clock
# times ocn_model_stage_times returns (the library's own sums: RungeKutta3 ticks between its stages).  A slot is sent only when
# its tables changed, so a drift constant in time costs nothing per step.  Not run: no Julia toolchain exists where this was written.
function set_stokes_drift!(model::RM, slot, t, sent)
    sw, grid, Nz = model.stokes_drift, model.grid, model.grid.Nz
    zc = [znode(Center(), k, grid) for k in 1:Nz]; zf = [znode(Face(), k, grid) for k in 1:Nz]
    tabs = (Float64[sw.∂z_uˢ(z, t) for z in zc], Float64[sw.∂z_vˢ(z, t) for z in zc], Float64[sw.∂z_uˢ(z, t) for z in zf],
            Float64[sw.∂z_vˢ(z, t) for z in zf], Float64[sw.∂t_uˢ(z, t) for z in zc], Float64[sw.∂t_vˢ(z, t) for z in zc])
    sent[slot + 1] == tabs && return nothing
    check(ccall((:ocn_model_set_stokes_drift, libocnhip), Cint, (Ptr{Cvoid}, Cint, Ptr{Float64}, Ptr{Float64}, Ptr{Float64}, Ptr{Float64},
                 Ptr{Float64}, Ptr{Float64}, Cint), handle(model), slot, tabs..., Nz), model.architecture.ctx)
    sent[slot + 1] = tabs
    return nothing
end
function refresh_stokes_drift!(model::RM, Δt)       # before ocn_time_step; model.auxiliary_fields.stokes_sent = Any[nothing, nothing, nothing]
    model.stokes_drift === nothing && return nothing
    times = zeros(3); n = Ref(Int32(0))
    check(ccall((:ocn_model_stage_times, libocnhip), Cint, (Ptr{Cvoid}, Cdouble, Ptr{Float64}, Ref{Int32}), handle(model), Δt, times, n))
    for s in 1:n[]
        set_stokes_drift!(model, s - 1, times[s], model.auxiliary_fields.stokes_sent)
    end
end
# the kernel-by-kernel verbs read the slot of the current stage: set_stokes_drift!(model, model.clock.stage - 1, model.clock.time, sent)
# before calculate_tendencies!(model)

# forcing = (u = Relaxation(...), T = (Relaxation(...), Forcing(func)), ...) (Forcings/relaxation.jl:80-84, continuous_forcing.jl:116-125,
# multiple_forcings.jl): G_phi += sigma (tau - phi) + F at phi's own nodes.  Accepted: Relaxation, ContinuousForcing without field
# dependencies, and tuples (MultipleForcings) of them; refused by name: field dependencies, DiscreteForcing, AdvectiveForcing, a second
# Relaxation of the same form on one field.  The functions stay in Julia and are evaluated on the nodes: numbers, GaussianMask{:z},
# LinearTarget{:z} and the default mask / target make the column form (three tables of Nz numbers per field and stage, at the clock
# times of ocn_model_stage_times, re-sent only when they changed); everything else the field form ((Nx, Ny, Nz) arrays, evaluated
# once; a probe at a second time must agree).  Not run: no Julia toolchain exists where this was written.
using Oceananigans.Forcings: ContinuousForcing, DiscreteForcing, MultipleForcings, AdvectiveForcing, Relaxation, GaussianMask, LinearTarget
forcing_members(f) = f isa MultipleForcings ? f.forcings : (f,)
is_relaxation(f) = f isa ContinuousForcing && f.func isa Relaxation
column_part(p) = p isa Number || p isa GaussianMask{:z} || p isa LinearTarget{:z} || p === Oceananigans.Forcings.onefunction ||
                 p === Oceananigans.Forcings.zerofunction
column_member(f) = is_relaxation(f) && column_part(f.func.mask) && column_part(f.func.target)
function forcing_plan(m)
    names = (:u, :v, :w, keys(m.tracers)...)
    plan = (column_fields = UInt32(0), field_fields = UInt32(0), members = Dict{Symbol, Any}())
    col, fld = UInt32(0), UInt32(0)
    for (i, n) in enumerate(names)
        haskey(m.forcing, n) || continue
        mem = [f for f in forcing_members(m.forcing[n]) if f !== Oceananigans.Forcings.zeroforcing && !(f isa Returns)]
        isempty(mem) && continue
        for f in mem
            f isa AdvectiveForcing && error("forcing of $n: AdvectiveForcing is outside the path")
            f isa DiscreteForcing && error("forcing of $n: discrete_form = true is outside the path")
            f isa ContinuousForcing || error("forcing of $n: $(typeof(f)) is outside the path")
            is_relaxation(f) || isempty(f.field_dependencies) || error("forcing of $n: field_dependencies are outside the path")
        end
        count(column_member, mem) <= 1 && count(f -> is_relaxation(f) && !column_member(f), mem) <= 1 ||
            error("forcing of $n: more than one Relaxation of the same form (two relaxations do not merge into one (sigma, tau) exactly)")
        any(column_member, mem) && (col |= UInt32(1) << (i - 1))
        any(!column_member, mem) && (fld |= UInt32(1) << (i - 1))
        plan.members[n] = (i - 1, mem)
    end
    return (column_fields = col, field_fields = fld, members = plan.members)
end
field_nodes(model, n) = (loc = n == :u ? (Face(), Center(), Center()) : n == :v ? (Center(), Face(), Center()) :
                               n == :w ? (Center(), Center(), Face()) : (Center(), Center(), Center());
                         g = model.grid; ([xnode(loc[1], i, g) for i in 1:g.Nx], [ynode(loc[2], j, g) for j in 1:g.Ny], [znode(loc[3], k, g) for k in 1:g.Nz]))
target_at(r, x, y, z, t) = r.target isa Number ? Float64(r.target) : Float64(r.target(x, y, z, t))
function set_forcing_columns!(model::RM, slot, t, sent)       # model.auxiliary_fields.forcing_plan / forcing_sent = Any[nothing, nothing, nothing]
    Nz = model.grid.Nz; tabs = Dict{Symbol, Any}()
    for (n, (f, mem)) in model.auxiliary_fields.forcing_plan.members
        any(column_member, mem) || continue
        x, y, z = field_nodes(model, n); r = first(filter(column_member, mem)).func
        tabs[n] = (Float64[r.rate * r.mask(x[1], y[1], zk) for zk in z], Float64[target_at(r, x[1], y[1], zk, t) for zk in z], zeros(Nz))
    end
    for (n, tab) in tabs
        sent[slot + 1] !== nothing && get(sent[slot + 1], n, nothing) == tab && continue
        check(ccall((:ocn_model_set_forcing_column, libocnhip), Cint, (Ptr{Cvoid}, Cint, Cint, Ptr{Float64}, Ptr{Float64}, Ptr{Float64}, Cint),
                    handle(model), model.auxiliary_fields.forcing_plan.members[n][1], slot, tab..., Nz), model.architecture.ctx)
    end
    sent[slot + 1] = tabs
    return nothing
end
function set_forcing_fields!(model::RM)                        # once, after construction: the field form is constant in time
    g = model.grid; t = model.clock.time
    for (n, (f, mem)) in model.auxiliary_fields.forcing_plan.members
        rest = filter(!column_member, mem); isempty(rest) && continue
        x, y, z = field_nodes(model, n)
        ev(fun) = Float64[fun(x[i], y[j], z[k]) for i in 1:g.Nx, j in 1:g.Ny, k in 1:g.Nz]
        rel = filter(is_relaxation, rest); fs = filter(!is_relaxation, rest)
        value(c, tt) = (X, Y, Z) -> c.parameters === nothing ? c.func(X, Y, Z, tt) : c.func(X, Y, Z, tt, c.parameters)
        σ = isempty(rel) ? nothing : ev((X, Y, Z) -> rel[1].func.rate * rel[1].func.mask(X, Y, Z))
        τ = isempty(rel) ? nothing : ev((X, Y, Z) -> target_at(rel[1].func, X, Y, Z, t))
        F = isempty(fs) ? nothing : sum(ev(value(c, t)) for c in fs)
        (isempty(rel) || τ == ev((X, Y, Z) -> target_at(rel[1].func, X, Y, Z, t + 0.7384))) && (isempty(fs) || F == sum(ev(value(c, t + 0.7384)) for c in fs)) ||
            error("forcing of $n: a forcing that depends on x or y and on time is outside the path (an (Nx, Ny, Nz) upload per stage)")
        ptr(a) = a === nothing ? Ptr{Float64}(C_NULL) : pointer(a)
        GC.@preserve σ τ F check(ccall((:ocn_model_set_forcing_field, libocnhip), Cint, (Ptr{Cvoid}, Cint, Ptr{Float64}, Ptr{Float64}, Ptr{Float64}, Cint, Cint, Cint),
                                       handle(model), f, ptr(σ), ptr(τ), ptr(F), g.Nx, g.Ny, g.Nz), model.architecture.ctx)
    end
end
function refresh_forcing!(model::RM, Δt)            # before ocn_time_step, like refresh_stokes_drift!
    isempty(model.auxiliary_fields.forcing_plan.members) && return nothing
    times = zeros(3); n = Ref(Int32(0))
    check(ccall((:ocn_model_stage_times, libocnhip), Cint, (Ptr{Cvoid}, Cdouble, Ptr{Float64}, Ref{Int32}), handle(model), Δt, times, n))
    for s in 1:n[]
        set_forcing_columns!(model, s - 1, times[s], model.auxiliary_fields.forcing_sent)
    end
end

# background_fields = (u = U, b = BackgroundField(B, parameters = p), ...) (Fields/background_fields.jl:5-75,
# nonhydrostatic_tendency_kernel_functions.jl:61-63,118-120,172-174,226-228): G_phi += -div(adv, (U, V, W), phi) - div(adv, (u, v, w), Phi).
# model.background_fields holds a FunctionField (or a user's Field, or a ZeroField) per member at the member's location; the kernels read
# it over the PARENT index range -- halo nodes at their extended coordinates -- so that is what is evaluated here.  Member f: 0, 1, 2 are
# U, V, W, 3 + t is the background of tracer t.  A FunctionField that gives the same column at two (x, y) is sent in the column form (one
# table over the parent levels per stage, may vary in time); everything else in the field form (the whole parent array, once; a probe at a
# second time must agree; a Field's parent array as it stands).  Not run: no Julia toolchain exists where this was written.
using Oceananigans.Fields: ZeroField, FunctionField
background_members(m) = ((:u, m.background_fields.velocities.u), (:v, m.background_fields.velocities.v), (:w, m.background_fields.velocities.w),
                         ((n, m.background_fields.tracers[n]) for n in keys(m.tracers))...)
parent_range(f, d) = (g = f.grid; N = size(g)[d]; H = halo_size(g)[d]; topology(g, d) === Flat ? (1:1) :
                      (1 - H):(N + H + (location(f)[d] === Face && topology(g, d) === Bounded ? 1 : 0)))
at_time(f::FunctionField, t) = FunctionField{location(f)...}(f.func, f.grid; clock = (time = t,), parameters = f.parameters)
column_of(f, i, j) = Float64[f[i, j, k] for k in parent_range(f, 3)]
is_column(f) = f isa FunctionField && column_of(f, 1, 1) == column_of(f, 1 + size(f.grid)[1] ÷ 3, 1 + size(f.grid)[2] ÷ 3)
function background_plan(m)
    col, fld = UInt32(0), UInt32(0); members = Dict{Symbol, Any}()
    for (i, (n, f)) in enumerate(background_members(m))
        f isa ZeroField && continue
        is_column(f) ? (col |= UInt32(1) << (i - 1)) : (fld |= UInt32(1) << (i - 1))
        members[n] = (i - 1, f)
    end
    return (column_members = col, field_members = fld, members = members)
end
function set_background_columns!(model::RM, slot, t, sent)    # model.auxiliary_fields.background_plan / background_sent = Any[nothing, nothing, nothing]
    plan = model.auxiliary_fields.background_plan; tabs = Dict{Symbol, Any}()
    for (n, (f, mem)) in plan.members
        (plan.column_members >> f) & 1 == 1 && (tabs[n] = column_of(at_time(mem, t), 1, 1))
    end
    for (n, tab) in tabs
        sent[slot + 1] !== nothing && get(sent[slot + 1], n, nothing) == tab && continue
        check(ccall((:ocn_model_set_background_column, libocnhip), Cint, (Ptr{Cvoid}, Cint, Cint, Ptr{Float64}, Cint),
                    handle(model), plan.members[n][1], slot, tab, length(tab)), model.architecture.ctx)
    end
    sent[slot + 1] = tabs
    return nothing
end
function set_background_fields!(model::RM)                    # once, after construction: the field form is constant in time
    plan = model.auxiliary_fields.background_plan; t = model.clock.time
    for (n, (f, mem)) in plan.members
        (plan.field_members >> f) & 1 == 1 || continue
        ev(fld) = Float64[fld[i, j, k] for i in parent_range(fld, 1), j in parent_range(fld, 2), k in parent_range(fld, 3)]
        a = mem isa FunctionField ? ev(at_time(mem, t)) : Array{Float64}(parent(mem))
        mem isa FunctionField && a != ev(at_time(mem, t + 0.7384)) &&
            error("background field $n: a background that depends on x or y and on time is outside the path (a parent-array upload per stage)")
        GC.@preserve a check(ccall((:ocn_model_set_background_field, libocnhip), Cint, (Ptr{Cvoid}, Cint, Ptr{Float64}, Cint, Cint, Cint),
                                   handle(model), f, a, size(a)...), model.architecture.ctx)
    end
end
function refresh_background!(model::RM, Δt)         # before ocn_time_step, like refresh_forcing!
    isempty(model.auxiliary_fields.background_plan.members) && return nothing
    times = zeros(3); n = Ref(Int32(0))
    check(ccall((:ocn_model_stage_times, libocnhip), Cint, (Ptr{Cvoid}, Cdouble, Ptr{Float64}, Ref{Int32}), handle(model), Δt, times, n))
    for s in 1:n[]
        set_background_columns!(model, s - 1, times[s], model.auxiliary_fields.background_sent)
    end
end

# TimeSteppers/quasi_adams_bashforth_2.jl:70-104 and runge_kutta_3.jl:81-152 -- preferred, coarsest overload
function time_step!(model::RM, Δt; euler=false)
    refresh_stokes_drift!(model, Δt)
    refresh_forcing!(model, Δt)
    refresh_background!(model, Δt)
    check(ccall((:ocn_time_step, libocnhip), Cint, (Ptr{Cvoid}, Cdouble, Cint), handle(model), Δt, euler), model.architecture.ctx)
    # clock mirrors ocn_clock (TimeSteppers/clock.jl:48-60)
    t = Ref(0.0); it = Ref(Int64(0)); st = Ref(Int32(0))
    ccall((:ocn_clock, libocnhip), Cint, (Ptr{Cvoid}, Ref{Float64}, Ref{Int64}, Ref{Int32}), handle(model), t, it, st)
    model.clock.time, model.clock.iteration, model.clock.stage = t[], it[], st[]
    return nothing
end

# finer-grained overloads, for callers that drive the phases themselves
update_state!(model::RM) = check(ccall((:ocn_update_state, libocnhip), Cint, (Ptr{Cvoid},), handle(model)))                        # update_nonhydrostatic_model_state.jl:14
calculate_tendencies!(model::RM) = check(ccall((:ocn_compute_tendencies, libocnhip), Cint, (Ptr{Cvoid},), handle(model)))           # calculate_nonhydrostatic_tendencies.jl:12
ab2_step!(model::RM, Δt, χ) = check(ccall((:ocn_ab2_step, libocnhip), Cint, (Ptr{Cvoid}, Cdouble, Cdouble), handle(model), Δt, χ))  # quasi_adams_bashforth_2.jl:116
rk3_substep!(model::RM, Δt, γ, ζ) = check(ccall((:ocn_rk3_substep, libocnhip), Cint, (Ptr{Cvoid}, Cdouble, Cdouble, Cdouble, Cint),
                                                handle(model), Δt, γ, something(ζ, 0.0), ζ !== nothing))                            # runge_kutta_3.jl:161
store_tendencies!(model::RM) = check(ccall((:ocn_store_tendencies, libocnhip), Cint, (Ptr{Cvoid},), handle(model)))                 # store_tendencies.jl:14
calculate_pressure_correction!(model::RM, Δt) = check(ccall((:ocn_pressure_correction, libocnhip), Cint, (Ptr{Cvoid}, Cdouble), handle(model), Δt))           # pressure_correction.jl:10
pressure_correct_velocities!(model::RM, Δt) = check(ccall((:ocn_pressure_correct_velocities, libocnhip), Cint, (Ptr{Cvoid}, Cdouble), handle(model), Δt))     # pressure_correction.jl:43

# set!(model; ...) : host arrays -> ocn_field_set_interior per field, then the epilogue (set_nonhydrostatic_model.jl:45-58)
function set!(model::RM; enforce_incompressibility=true, kwargs...)
    for (name, value) in kwargs
        host = Array{Float64}(undef, size(getproperty(merge(model.velocities, model.tracers), name)))
        set!(CPUField(name, model), value); host .= interior(CPUField(name, model))     # stage on the CPU exactly like Fields/set!.jl:21-27
        check(ccall((:ocn_field_set_interior, libocnhip), Cint, (Ptr{Cvoid}, Cint, Ptr{Float64}), handle(model), field_id(model, name), host))
    end
    check(ccall((:ocn_set_epilogue, libocnhip), Cint, (Ptr{Cvoid}, Cint), handle(model), enforce_incompressibility))
end

# Output / checkpoint fetch (OutputWriters/fetch_output.jl:26, checkpointer.jl:158-180): parent arrays incl. G^n, G^-
function arch_array(::CPU, a::OffsetArray{T, 3, <:ROCArray}) where T
    host = Array{T}(undef, size(parent(a)))
    # the owning model + field id travel with the wrapper in the real shim; shown here for one field:
    # check(ccall((:ocn_field_download, libocnhip), Cint, (Ptr{Cvoid}, Cint, Ptr{Float64}), model_handle, field_id, host))
    return OffsetArray(host, a.offsets...)
end

# Which kernels serve a model (and why not the fastest ones): ocn_model_path(handle, buf, n) -> String, for `show(model)`.
kernel_path(model::RM) = (buf = Vector{UInt8}(undef, 256);
                          check(ccall((:ocn_model_path, libocnhip), Cint, (Ptr{Cvoid}, Ptr{UInt8}, Csize_t), handle(model), buf, 256));
                          unsafe_string(pointer(buf)))

# Checkpoint / restart (OutputWriters/checkpointer.jl:158-265): download the parent arrays of u, v, w, tracers, G^n, G^- and
# the clock; restore with ocn_field_upload + ocn_set_clock(time, iteration, previous_dt) + update_state!.  Continuing from
# the restored state is bit-identical to the uninterrupted run (tests/test_model_contracts.py, all four stepper / topology pairs).

# Distributed: MultiArch(ROCmGPU(); ranks=(1, 1, R)) -> ocn_comm_init(ctx, rank, R, id) with the 128-byte id of
# ocn_comm_unique_id broadcast over MPI (Distributed/multi_architectures.jl:20-47); everything else is unchanged.
# Before the blocking ocn_comm_init every rank calls ocn_comm_probe(ctx, rank, R, id0, timeout_s) with an id of its own and the
# ranks MPI.Allreduce(min) the return codes: a rank whose RCCL cannot start then stops everybody instead of hanging them.
#
# HydrostaticFreeSurfaceModel, first slice (Models/HydrostaticFreeSurfaceModels/split_explicit_free_surface*.jl):
#   struct ROCmSplitExplicit; grid::Ptr{Cvoid}; sefs::Ptr{Cvoid}; end                      # ocn_hgrid_create + ocn_sefs_create
#   FreeSurface(fs::SplitExplicitFreeSurface, velocities, grid) on a ROCmGPU grid -> fields aliased from ocn_sefs_field(sefs, 0:10)
#   ab2_step_free_surface!(fs, model, Δt, χ, _) = check(ccall((:ocn_sefs_step, libocnhip), Cint,
#       (Ptr{Cvoid}, Ptr{Cvoid}, Ptr{Cvoid}, Ptr{Cvoid}, Ptr{Cvoid}, Cdouble, Cdouble), fs.sefs, Gⁿ.u, Gⁿ.v, G⁻.u, G⁻.v, Δt, χ))
#   barotropic_split_explicit_corrector!(u, v, fs, grid) = check(ccall((:ocn_sefs_corrector, libocnhip), Cint,
#       (Ptr{Cvoid}, Ptr{Cvoid}, Ptr{Cvoid}), fs.sefs, hfield(u), hfield(v)))
#   ImplicitFreeSurface(; solver_method = :PreconditionedConjugateGradient, preconditioner = nothing) (implicit_free_surface.jl):
#   struct ROCmImplicit; grid::Ptr{Cvoid}; ifs::Ptr{Cvoid}; end     # ocn_ifs_create(grid, g, reltol, abstol, maxiter) (1e-7, 0, Nx Ny)
#   FreeSurface(fs::ImplicitFreeSurface, velocities, grid) on a ROCmGPU grid -> η, ∫ᶻQ, rhs aliased from ocn_ifs_field(ifs, 0:5);
#       any other solver_method or a preconditioner throws ArgumentError (the library has the unpreconditioned PCG only)
#   ab2_step_free_surface!(fs::ImplicitFreeSurface, model, Δt, χ, _) = check(ccall((:ocn_ifs_step, libocnhip), Cint,
#       (Ptr{Cvoid}, Ptr{Cvoid}, Ptr{Cvoid}, Cdouble), fs.ifs, hfield(model.velocities.u), hfield(model.velocities.v), Δt))
#   solver_method = :FastFourierTransform, or :Default on a regular RectilinearGrid: fs.ifs from ocn_ifs_create_fft(grid, g) instead (flat
#       bottom, <= 4096 points per direction; settings ignored as the reference ignores them; ocn_ifs_field(ifs, 3:4) are C_NULL: no ∫ᶻA;
#       ocn_ifs_method(ifs, method, x_path, y_path) tells 0 PCG / 1 FFT and 0 fast / 1 direct transform per direction)
#   the model handle: ocn_hydro_create_implicit(desc, fs.ifs, h) with desc.free_surface = C_NULL; solver.iteration = ocn_ifs_iterations
# closure = SmagorinskyLilly(C, Cb, Pr) (or (SmagorinskyLilly, ScalarDiffusivity)) on the NonhydrostaticModel: ocn_model(arch, gridh, m) calls
#   ocn_model_create_smagorinsky_lilly(gridh, desc, Ref(SmagDesc(C, Cb, Pr...)), h) with desc.closure = NONE (or SCALAR + nu / kappa); model.diffusivity_fields.νₑ wraps OCN_F_NU
#
# Launch-bound models (config 1) are replayed from hipGraphs inside ocn_time_step; ocn_model_graph_replays(handle, n, active)
# reports it.  The library reports OCN_ABI_VERSION through ocn_abi_version(): __init__ compares it with 5.
function __init__()
    v = ccall((:ocn_abi_version, libocnhip), Cint, ())
    v == 5 || error("libocnhip reports ABI version $v; this shim is written for 5")
end

end # module
