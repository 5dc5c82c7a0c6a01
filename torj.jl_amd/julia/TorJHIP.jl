# TorJHIP.jl -- drop-in GPU back end for TorJ.jl's ray-tracing path (make_ray /
# make_beam, src/solve.jl) on AMD MI355X, through the C ABI of libtorj_hip.so
# (include/torj_hip.h).  Kept deliberately thin: argument marshalling only.
#
# Usage (see INTEGRATION.md):
#     using TorJ, TorJHIP
#     TorJHIP.abs_Al_init(24)
#     plasma = TorJ.Plasma(R, Z, psi_norm, psi_prof, ne, Te, Br, Bz, Bphi, eq_psi, eq_vol)
#     s, u, P, dP_dV, P_dep = TorJHIP.make_ray(plasma, x0, N0, f, 1, 0.4, psi_dP_dV)
#     out = TorJHIP.make_beam(plasma, r, phi, z, tor, pol, spot, inv_curv, f, 1, 1.0,
#                             psi_dP_dV; N_rings=92, min_azimuthal_points=11, n_gpus=8)
# A TorJ.Plasma is converted once (GPUPlasma(plasma): its Interpolations.jl
# B-spline coefficients go to the GPU as they are) and cached per object.
#
# Untested in this repository's container (no Julia toolchain); the same ABI is
# exercised by the Python ctypes mirror in torj.jl_amd/torj_hip.
module TorJHIP

import TorJ

const libtorj = get(ENV, "TORJ_HIP_LIB", joinpath(@__DIR__, "..", "build", "libtorj_hip.so"))
const ABI_VERSION = 8  # include/torj_hip.h TORJ_ABI_VERSION

function __init__()
    v = ccall((:torj_abi_version, libtorj), Cint, ())
    v == ABI_VERSION || error("libtorj_hip.so at $libtorj has ABI version $v, TorJHIP expects $ABI_VERSION")
end

struct TraceCfg              # torj_trace_cfg
    omega::Float64
    mode::Cint
    ds::Float64
    n_steps::Cint
    chunk_steps::Cint
    psi_exit::Float64
    P_min::Float64
    absorption::Cint         # 0 none, 1 abs_Albajar_fast, 2 / 3 warm alpha (iwarm 1 / 3)
    traj_stride::Cint
    deposition::Cint         # 0: binned, 1: power_deposition_profile (src/plasma.jl:91-151)
    integrator::Cint         # 0: fixed RK4; 1: the reference's adaptive solve() (Tsit5)
    abstol::Float64
    reltol::Float64
    s_max::Float64
    n_chunks::Cint
end

check(rc) = rc == 0 || error(unsafe_string(ccall((:torj_last_error, libtorj), Cstring, ())))

"""abs_Al_init(N) -- src/absorption.jl:1-7"""
abs_Al_init(n::Integer) = check(ccall((:torj_abs_al_init, libtorj), Cint, (Cint,), n))

mutable struct GPUPlasma
    h::Ptr{Cvoid}
    psi_prof_max::Float64
    nR::Int                  # the handle's grid size (update! keeps it)
    nZ::Int
    function GPUPlasma(h::Ptr{Cvoid}, psi_prof_max::Float64, nR::Integer, nZ::Integer)
        p = new(h, psi_prof_max, nR, nZ)
        finalizer(x -> ccall((:torj_plasma_destroy, libtorj), Cint, (Ptr{Cvoid},), x.h), p)
        return p
    end
end

"""GPUPlasma from the raw maps -- the arguments of TorJ.Plasma (src/plasma.jl:30-32);
the B-spline prefilter runs in the library."""
function GPUPlasma(R::Vector{Float64}, Z::Vector{Float64}, psi_norm::Matrix{Float64},
                   psi_prof::Vector{Float64}, ne::Vector{Float64}, Te::Vector{Float64},
                   Br::Matrix{Float64}, Bz::Matrix{Float64}, Bphi::Matrix{Float64},
                   eq_psi::Vector{Float64}, eq_vol::Vector{Float64}; device::Integer=0)
    h = Ref{Ptr{Cvoid}}(C_NULL)
    # Julia matrices are (nR, nZ) column-major: exactly the ABI layout
    check(ccall((:torj_plasma_create, libtorj), Cint,
                (Cint, Cint, Ptr{Float64}, Ptr{Float64}, Ptr{Float64}, Cint, Ptr{Float64},
                 Ptr{Float64}, Ptr{Float64}, Ptr{Float64}, Ptr{Float64}, Ptr{Float64}, Cint,
                 Ptr{Float64}, Ptr{Float64}, Cint, Ptr{Ptr{Cvoid}}),
                length(R), length(Z), R, Z, psi_norm, length(psi_prof), psi_prof, ne, Te,
                Br, Bz, Bphi, length(eq_psi), eq_psi, eq_vol, device, h))
    return GPUPlasma(h[], maximum(psi_prof), length(R), length(Z))
end

# Interpolations.jl: cubic_spline_interpolation(ranges, A; extrapolation_bc=Line())
# is extrapolate(scale(interpolate(A, BSpline(Cubic(Line(OnGrid())))), ranges...), Line());
# .itp is the ScaledInterpolation (its .ranges), .itp.itp the BSplineInterpolation
# whose padded coefficient OffsetArray has parent (n+2) x (m+2).
_coefs(spl) = Array{Float64}(parent(spl.itp.itp.coefs))
_ranges(spl) = spl.itp.ranges

"""GPUPlasma(plasma::TorJ.Plasma) -- the TorJ object itself (src/plasma.jl:2-14): its six
2-D splines' coefficients (psi, ln ne, ln Te, Br, Bz, Bphi) and the 1-D volume spline
go to the GPU unchanged (torj_plasma_create_from_coefs), so the GPU evaluates exactly
the splines TorJ built."""
function GPUPlasma(p::TorJ.Plasma; device::Integer=0)
    rR, rZ = _ranges(p.psi_norm_spline)
    c = [_coefs(getfield(p, f)) for f in (:psi_norm_spline, :ne_spline, :Te_spline,
                                           :Br_spline, :Bz_spline, :Bϕ_spline)]
    all(size(x) == (length(rR) + 2, length(rZ) + 2) for x in c) ||
        throw(ArgumentError("TorJ.Plasma splines are not on one (R, Z) grid"))
    rv = _ranges(p.volume_psi_spline)[1]
    cv = _coefs(p.volume_psi_spline)
    h = Ref{Ptr{Cvoid}}(C_NULL)
    check(ccall((:torj_plasma_create_from_coefs, libtorj), Cint,
                (Cint, Cint, Float64, Float64, Float64, Float64, Ptr{Float64}, Ptr{Float64},
                 Ptr{Float64}, Ptr{Float64}, Ptr{Float64}, Ptr{Float64}, Cint, Float64, Float64,
                 Ptr{Float64}, Float64, Cint, Ptr{Ptr{Cvoid}}),
                length(rR), length(rZ), first(rR), last(rR), first(rZ), last(rZ), c[1], c[2],
                c[3], c[4], c[5], c[6], length(rv), first(rv), last(rv), cv,
                Float64(p.psi_prof_max), device, h))
    return GPUPlasma(h[], Float64(p.psi_prof_max), length(rR), length(rZ))
end

"""update!(h, plasma::TorJ.Plasma; stream=C_NULL) -- the live handle `h` takes `plasma`'s
splines (torj_plasma_update_from_coefs): a transport loop keeps one handle, with its
workspaces, streams and replicas, and refills it between traces.  The (R, Z) grid must have
the size `h` was built with; its ranges may differ.  After the handle's first GPU use the
copy and the rebuild of the cell table are enqueued on `stream` without synchronisation."""
function update!(h::GPUPlasma, p::TorJ.Plasma; stream::Ptr{Cvoid}=C_NULL)
    rR, rZ = _ranges(p.psi_norm_spline)
    c = [_coefs(getfield(p, f)) for f in (:psi_norm_spline, :ne_spline, :Te_spline,
                                           :Br_spline, :Bz_spline, :Bϕ_spline)]
    all(size(x) == (length(rR) + 2, length(rZ) + 2) for x in c) ||
        throw(ArgumentError("TorJ.Plasma splines are not on one (R, Z) grid"))
    (length(rR), length(rZ)) == (h.nR, h.nZ) ||
        throw(ArgumentError("update! keeps the handle's grid size $((h.nR, h.nZ)), got $((length(rR), length(rZ)))"))
    rv = _ranges(p.volume_psi_spline)[1]
    cv = _coefs(p.volume_psi_spline)
    check(ccall((:torj_plasma_update_from_coefs, libtorj), Cint,
                (Ptr{Cvoid}, Float64, Float64, Float64, Float64, Ptr{Float64}, Ptr{Float64},
                 Ptr{Float64}, Ptr{Float64}, Ptr{Float64}, Ptr{Float64}, Cint, Float64, Float64,
                 Ptr{Float64}, Float64, Ptr{Cvoid}),
                h.h, first(rR), last(rR), first(rZ), last(rZ), c[1], c[2], c[3], c[4], c[5], c[6],
                length(rv), first(rv), last(rv), cv, Float64(p.psi_prof_max), stream))
    h.psi_prof_max = Float64(p.psi_prof_max)
    return h
end

"""update_gpu!(h, R, Z, psi_norm, psi_prof, ne, Te, Br, Bz, Bphi, eq_psi, eq_vol; stream=C_NULL) -- the
raw maps of `GPUPlasma(R, Z, ...)` on the live handle `h` (torj_plasma_update_gpu): the six 2-D
B-spline prefilters run on the GPU in `stream`'s order, the 1-D parts on the host.  The host arrays
are consumed when the call returns; nothing synchronises."""
function update_gpu!(h::GPUPlasma, R::Vector{Float64}, Z::Vector{Float64}, psi_norm::Matrix{Float64},
                     psi_prof::Vector{Float64}, ne::Vector{Float64}, Te::Vector{Float64},
                     Br::Matrix{Float64}, Bz::Matrix{Float64}, Bphi::Matrix{Float64},
                     eq_psi::Vector{Float64}, eq_vol::Vector{Float64}; stream::Ptr{Cvoid}=C_NULL)
    (length(R), length(Z)) == (h.nR, h.nZ) ||
        throw(ArgumentError("update_gpu! keeps the handle's grid size $((h.nR, h.nZ)), got $((length(R), length(Z)))"))
    all(size(x) == (h.nR, h.nZ) for x in (psi_norm, Br, Bz, Bphi)) ||
        throw(ArgumentError("update_gpu!: the 2-D maps must be $((h.nR, h.nZ))"))
    check(ccall((:torj_plasma_update_gpu, libtorj), Cint,
                (Ptr{Cvoid}, Ptr{Float64}, Ptr{Float64}, Ptr{Float64}, Cint, Ptr{Float64},
                 Ptr{Float64}, Ptr{Float64}, Ptr{Float64}, Ptr{Float64}, Ptr{Float64}, Cint,
                 Ptr{Float64}, Ptr{Float64}, Ptr{Cvoid}),
                h.h, R, Z, psi_norm, length(psi_prof), psi_prof, ne, Te, Br, Bz, Bphi,
                length(eq_psi), eq_psi, eq_vol, stream))
    h.psi_prof_max = maximum(psi_prof)
    return h
end

"""update_profiles_gpu!(h, psi_prof, ne, Te; stream=C_NULL) -- new kinetic profiles on the
equilibrium `h` last got as node data (torj_plasma_update_profiles_gpu): make_2d_prof_spline's
node map and the two prefilters run on the GPU, from the psi nodes the handle keeps there."""
function update_profiles_gpu!(h::GPUPlasma, psi_prof::Vector{Float64}, ne::Vector{Float64},
                              Te::Vector{Float64}; stream::Ptr{Cvoid}=C_NULL)
    length(psi_prof) == length(ne) == length(Te) ||
        throw(ArgumentError("psi_prof, ne and Te must have one length"))
    check(ccall((:torj_plasma_update_profiles_gpu, libtorj), Cint,
                (Ptr{Cvoid}, Cint, Ptr{Float64}, Ptr{Float64}, Ptr{Float64}, Ptr{Cvoid}),
                h.h, length(psi_prof), psi_prof, ne, Te, stream))
    h.psi_prof_max = maximum(psi_prof)
    return h
end

"""update_device!(h, R, Z, d_psi_norm, psi_prof, ne, Te, d_Br, d_Bz, d_Bphi, eq_psi, eq_vol;
stream=C_NULL) -- update_gpu! with the four 2-D maps as device pointers on the handle's device
((nR, nZ) Float64, column-major, e.g. `pointer` of a ROCArray), read in `stream`'s order
(torj_plasma_update_device): they must stay unchanged until the stream has passed the call."""
function update_device!(h::GPUPlasma, R::Vector{Float64}, Z::Vector{Float64}, d_psi_norm::Ptr{Float64},
                        psi_prof::Vector{Float64}, ne::Vector{Float64}, Te::Vector{Float64},
                        d_Br::Ptr{Float64}, d_Bz::Ptr{Float64}, d_Bphi::Ptr{Float64},
                        eq_psi::Vector{Float64}, eq_vol::Vector{Float64}; stream::Ptr{Cvoid}=C_NULL)
    (length(R), length(Z)) == (h.nR, h.nZ) ||
        throw(ArgumentError("update_device! keeps the handle's grid size $((h.nR, h.nZ)), got $((length(R), length(Z)))"))
    check(ccall((:torj_plasma_update_device, libtorj), Cint,
                (Ptr{Cvoid}, Ptr{Float64}, Ptr{Float64}, Ptr{Float64}, Cint, Ptr{Float64},
                 Ptr{Float64}, Ptr{Float64}, Ptr{Float64}, Ptr{Float64}, Ptr{Float64}, Cint,
                 Ptr{Float64}, Ptr{Float64}, Ptr{Cvoid}),
                h.h, R, Z, d_psi_norm, length(psi_prof), psi_prof, ne, Te, d_Br, d_Bz, d_Bphi,
                length(eq_psi), eq_psi, eq_vol, stream))
    h.psi_prof_max = maximum(psi_prof)
    return h
end

# one GPU copy per TorJ.Plasma object (make_ray / make_beam on TorJ's own type)
const _gpu_cache = IdDict{Any,GPUPlasma}()
const _gpu_lock = ReentrantLock()
gpu_plasma(p::TorJ.Plasma) = lock(() -> get!(() -> GPUPlasma(p), _gpu_cache, p), _gpu_lock)

"""first_point + vacuum_plasma_refraction for n rays (x0, N0: n x 3), on the GPU."""
function ray_entry(p::GPUPlasma, x0::Matrix{Float64}, N0::Matrix{Float64}, omega, mode)
    n = size(x0, 1)
    xp, Np, s0, st = zeros(n, 3), zeros(n, 3), zeros(n), zeros(Cint, n)
    check(ccall((:torj_ray_entry_gpu, libtorj), Cint,
                (Ptr{Cvoid}, Cint, Ptr{Float64}, Ptr{Float64}, Float64, Cint, Ptr{Float64},
                 Ptr{Float64}, Ptr{Float64}, Ptr{Cint}),
                p.h, n, x0, N0, omega, mode, xp, Np, s0, st))
    return xp, Np, s0, st
end

function trace(p::GPUPlasma, cfg::TraceCfg, x0::Matrix{Float64}, N0::Matrix{Float64},
               w::Vector{Float64}, psi_grid::Vector{Float64}, x_launch::Matrix{Float64},
               s0::Vector{Float64}; n_gpus::Integer=1, n_shards::Integer=0)
    n = size(x0, 1)
    n_save = cfg.traj_stride > 0 ? cfg.n_steps ÷ cfg.traj_stride : 0
    state, status, steps = zeros(n, 7), zeros(Cint, n), zeros(Cint, n)
    dP, Pdep = zeros(length(psi_grid) + 1), zeros(n)
    traj = n_save > 0 ? zeros(n, 5, n_save) : zeros(0, 5, 0)
    GC.@preserve x0 N0 w psi_grid x_launch s0 begin
        # make_beam's fan-out over n_gpus devices + the RCCL reduce of dP_shell
        check(ccall((:torj_trace_beam, libtorj), Cint,
                    (Ptr{Cvoid}, Ref{TraceCfg}, Cint, Ptr{Float64}, Ptr{Float64}, Ptr{Float64},
                     Cint, Ptr{Float64}, Ptr{Float64}, Ptr{Float64}, Ptr{Float64}, Ptr{Cint},
                     Ptr{Cint}, Ptr{Float64}, Ptr{Float64}, Ptr{Float64}, Cint, Cint),
                    p.h, cfg, n, x0, N0, w, length(psi_grid), psi_grid, x_launch, s0, state,
                    status, steps, dP, Pdep, n_save > 0 ? traj : C_NULL, n_gpus, n_shards))
    end
    return state, status, steps, dP, Pdep, traj
end

# who took part in the last make_beam reduce over n_gpus replicas (ABI 8): each
# replica's HIP device and its RCCL communicator's rank count and rank (0 / -1
# where no communicator exists)
function beam_comm_info(p::GPUPlasma, n_gpus::Integer)
    dev, nranks, rank = zeros(Cint, n_gpus), zeros(Cint, n_gpus), zeros(Cint, n_gpus)
    check(ccall((:torj_beam_comm_info, libtorj), Cint,
                (Ptr{Cvoid}, Cint, Ptr{Cint}, Ptr{Cint}, Ptr{Cint}), p.h, n_gpus, dev, nranks, rank))
    return (device=dev, rccl_nranks=nranks, rccl_rank=rank)
end

function shell_volumes(p::GPUPlasma, g::Vector{Float64})
    dV = zeros(length(g) - 1)
    check(ccall((:torj_shell_volumes, libtorj), Cint, (Ptr{Cvoid}, Cint, Ptr{Float64}, Ptr{Float64}),
                p.h, length(g), g, dV))
    return dV
end

"""power_deposition_profile -- same signature and return tuple as
TorJ.power_deposition_profile (src/plasma.jl:91-151), on the GPU: psi at x from the
plasma's spline, the not-a-knot fits, Dierckx.roots (maxn = 8) pairing and the
outside-in walk.  Returns (dP_dV, P)."""
function power_deposition_profile(p::GPUPlasma, s::Vector{Float64}, x::Vector{Vector{Float64}},
                                  dP_ds::Vector{Float64}, psi_dP_dV::Vector{Float64})
    n = length(s)
    (length(x) == n && length(dP_ds) == n) || throw(DimensionMismatch("s, x, dP_ds lengths differ"))
    xm = Matrix{Float64}(undef, n, 3)  # n x 3 column-major = the ABI's component-major 3 x n
    for i in 1:n, c in 1:3
        xm[i, c] = x[i][c]
    end
    dP_dV, P = zeros(length(psi_dP_dV)), zeros(1)
    np = Cint[n]
    check(ccall((:torj_power_deposition_profile, libtorj), Cint,
                (Ptr{Cvoid}, Cint, Ptr{Cint}, Ptr{Float64}, Ptr{Float64}, Ptr{Float64}, Cint,
                 Ptr{Float64}, Ptr{Float64}, Ptr{Float64}),
                p.h, 1, np, s, xm, dP_ds, length(psi_dP_dV), psi_dP_dV, dP_dV, P))
    return dP_dV, P[1]
end
power_deposition_profile(p::TorJ.Plasma, args...) = power_deposition_profile(gpu_plasma(p), args...)

"""make_ray -- same signature and return tuple as TorJ.make_ray (src/solve.jl:135-181)."""
function make_ray(p::GPUPlasma, x0::AbstractVector, N_vacuum::AbstractVector, f::Real,
                  mode::Integer, s_max::Float64, psi_dP_dV::AbstractVector; ds::Float64=1e-4,
                  deposition::Integer=1, integrator::Integer=0, absorption::Integer=1)
    ω = 2π * f
    xp, Np, s0, st = ray_entry(p, reshape(collect(Float64, x0), 1, 3),
                               reshape(collect(Float64, N_vacuum), 1, 3), ω, mode)
    st[1] == 0 || throw(AssertionError("ray entry failed (status $(st[1]))"))
    n_steps = max(1, round(Int, s_max / ds))
    cap = integrator == 1 ? 2n_steps + 400 : n_steps
    cfg = TraceCfg(ω, mode, ds, cap, max(1, n_steps ÷ 100), 1.0, 1e-6, absorption, 1, deposition,
                   integrator, 1e-6, 1e-6, s_max, 100)
    g = collect(Float64, psi_dP_dV)
    xl = reshape(collect(Float64, x0), 1, 3)
    state, status, steps, dP, Pdep, traj = trace(p, cfg, xp, Np, ones(1), g, xl, s0)
    k = steps[1]
    s = vcat(0.0, s0[1], traj[1, 5, 1:k])
    u = vcat([collect(Float64, x0)], [xp[1, :]], [traj[1, 1:3, i] for i in 1:k])
    P_beam = vcat(1.0, 1.0, exp.(-traj[1, 4, 1:k]))
    dP_dV = zeros(length(g))
    dP_dV[1:end-1] .= dP[1:end-2] ./ shell_volumes(p, g)
    return s, u, P_beam, dP_dV, Pdep[1]
end
make_ray(p::TorJ.Plasma, args...; kw...) = make_ray(gpu_plasma(p), args...; kw...)

# a launcher's fan (make_beam, make_beams): the IMAS angles to a direction, then
# launch_peripheral_rays from (r, phi, z) -- positions and directions n x 3, weights n
function _launch_fan(r, phi, z, tor, pol, spot, inv_curv, f, N_rings, min_azimuthal_points,
                     normalize_weight_sum)
    N0 = zeros(3)
    ccall((:torj_pol_tor_angles_2_vector, libtorj), Cvoid, (Float64, Float64, Ptr{Float64}),
          pol, tor, N0)
    x0 = [r * cos(phi), r * sin(phi), z]
    nr = Ref{Cint}(0)
    check(ccall((:torj_launch_peripheral_rays, libtorj), Cint,
                (Ptr{Float64}, Ptr{Float64}, Float64, Float64, Float64, Cint, Cint, Cint, Ref{Cint},
                 Ptr{Float64}, Ptr{Float64}, Ptr{Float64}),
                x0, N0, spot, inv_curv, f, N_rings, min_azimuthal_points, normalize_weight_sum, nr,
                C_NULL, C_NULL, C_NULL))
    n = nr[]
    pos, dirs, w = zeros(n, 3), zeros(n, 3), zeros(n)
    check(ccall((:torj_launch_peripheral_rays, libtorj), Cint,
                (Ptr{Float64}, Ptr{Float64}, Float64, Float64, Float64, Cint, Cint, Cint, Ref{Cint},
                 Ptr{Float64}, Ptr{Float64}, Ptr{Float64}),
                x0, N0, spot, inv_curv, f, N_rings, min_azimuthal_points, normalize_weight_sum, nr,
                pos, dirs, w))
    return pos, dirs, w
end

"""make_beam -- same signature and return tuple as TorJ.make_beam (src/solve.jl:209-242);
the launch fan and IMAS angles on the host, every ray on the GPU(s): n_gpus devices of
this process (torj_trace_beam), dP_shell summed across them by RCCL.  traj_stride keeps
every traj_stride-th step of each ray (1 = all, as the reference) plus its final state."""
function make_beam(p::GPUPlasma, r, phi, z, tor, pol, spot, inv_curv, f, mode::Integer,
                   s_max::Float64, psi_dP_dV::Vector{Float64}; ds::Float64=1e-4,
                   N_rings::Integer=3, min_azimuthal_points::Integer=5,
                   normalize_weight_sum::Bool=true, deposition::Integer=1,
                   integrator::Integer=0, absorption::Integer=1, traj_stride::Integer=1,
                   n_gpus::Integer=1)
    pos, dirs, w = _launch_fan(r, phi, z, tor, pol, spot, inv_curv, f, N_rings, min_azimuthal_points,
                               normalize_weight_sum)
    n = length(w)
    ω = 2π * f
    xp, Np, s0, st = ray_entry(p, pos, dirs, ω, mode)
    all(st .== 0) || throw(AssertionError("ray entry failed for $(count(st .!= 0)) rays"))
    n_steps = max(1, round(Int, s_max / ds))
    cap = integrator == 1 ? 2n_steps + 400 : n_steps
    traj_stride >= 1 || throw(ArgumentError("traj_stride must be >= 1"))
    # checked before tracing: the adaptive integrator's final state is no saved sample
    (integrator == 1 && traj_stride > 1) &&
        throw(ArgumentError("integrator = 1 (adaptive) needs traj_stride = 1"))
    cfg = TraceCfg(ω, mode, ds, cap, max(1, n_steps ÷ 100), 1.0, 1e-6, absorption, traj_stride,
                   deposition, integrator, 1e-6, 1e-6, s_max, 100)
    state, status, steps, dP, Pdep, traj = trace(p, cfg, xp, Np, w, psi_dP_dV, pos, s0;
                                                 n_gpus=n_gpus)
    dP_dV = zeros(length(psi_dP_dV))
    dP_dV[1:end-1] .= dP[1:end-2] ./ shell_volumes(p, psi_dP_dV)
    arc_lengths, trajectories, ray_powers = Vector{Vector{Float64}}(), Vector{Vector{Vector{Float64}}}(), Vector{Vector{Float64}}()
    for i in 1:n
        k = steps[i] ÷ traj_stride
        s_i, x_i, τ_i = traj[i, 5, 1:k], [traj[i, 1:3, j] for j in 1:k], traj[i, 4, 1:k]
        if steps[i] % traj_stride != 0  # the final state is not a saved sample
            # fma: the single-rounding s0 + steps ds the trajectory kernel stores
            push!(s_i, fma(Float64(steps[i]), ds, s0[i])); push!(x_i, state[i, 1:3]); push!(τ_i, state[i, 7])
        end
        push!(arc_lengths, vcat(0.0, s0[i], s_i))
        push!(trajectories, vcat([pos[i, :]], [xp[i, :]], x_i))
        push!(ray_powers, vcat(1.0, 1.0, exp.(-τ_i)))
    end
    return arc_lengths, trajectories, ray_powers, dP_dV, dP[end], w
end
make_beam(p::TorJ.Plasma, args...; kw...) = make_beam(gpu_plasma(p), args...; kw...)

# ---- many beams of differing frequency and mode in one launch (torj_trace_beams) ----
# beam b owns rays beam_off[b] + 1 : beam_off[b + 1] (beam_off: 0-based offsets, length B + 1)

"""ray_entry for the concatenated rays of B beams, ray i with its beam's omega and mode."""
function ray_entry_beams(p::GPUPlasma, beam_off::Vector{Cint}, omega::Vector{Float64},
                         mode::Vector{Cint}, x0::Matrix{Float64}, N0::Matrix{Float64})
    n = size(x0, 1)
    xp, Np, s0, st = zeros(n, 3), zeros(n, 3), zeros(n), zeros(Cint, n)
    check(ccall((:torj_ray_entry_beams_gpu, libtorj), Cint,
                (Ptr{Cvoid}, Cint, Ptr{Cint}, Ptr{Float64}, Ptr{Cint}, Ptr{Float64}, Ptr{Float64},
                 Ptr{Float64}, Ptr{Float64}, Ptr{Float64}, Ptr{Cint}),
                p.h, length(omega), beam_off, omega, mode, x0, N0, xp, Np, s0, st))
    return xp, Np, s0, st
end

"""trace for B beams in one launch: cfg.omega and cfg.mode are ignored, dP has one row of
length(psi_grid) + 1 per beam (returned as a (length(psi_grid) + 1) x B matrix)."""
function trace_beams(p::GPUPlasma, cfg::TraceCfg, beam_off::Vector{Cint}, omega::Vector{Float64},
                     mode::Vector{Cint}, x0::Matrix{Float64}, N0::Matrix{Float64},
                     w::Vector{Float64}, psi_grid::Vector{Float64}, x_launch::Matrix{Float64},
                     s0::Vector{Float64})
    n, B = size(x0, 1), length(omega)
    n_save = cfg.traj_stride > 0 ? cfg.n_steps ÷ cfg.traj_stride : 0
    state, status, steps = zeros(n, 7), zeros(Cint, n), zeros(Cint, n)
    dP, Pdep = zeros(length(psi_grid) + 1, B), zeros(n)
    traj = n_save > 0 ? zeros(n, 5, n_save) : zeros(0, 5, 0)
    GC.@preserve beam_off omega mode x0 N0 w psi_grid x_launch s0 begin
        check(ccall((:torj_trace_beams, libtorj), Cint,
                    (Ptr{Cvoid}, Ref{TraceCfg}, Cint, Ptr{Cint}, Ptr{Float64}, Ptr{Cint}, Ptr{Float64},
                     Ptr{Float64}, Ptr{Float64}, Cint, Ptr{Float64}, Ptr{Float64}, Ptr{Float64},
                     Ptr{Float64}, Ptr{Cint}, Ptr{Cint}, Ptr{Float64}, Ptr{Float64}, Ptr{Float64}),
                    p.h, cfg, B, beam_off, omega, mode, x0, N0, w, length(psi_grid), psi_grid,
                    x_launch, s0, state, status, steps, dP, Pdep, n_save > 0 ? traj : C_NULL))
    end
    return state, status, steps, dP, Pdep, traj
end

"""make_beams(plasma, launchers, s_max, psi_dP_dV; ...) -- one make_beam tuple per launcher,
every launcher's rays in ONE launch.  `launchers`: tuples (r, phi, z, tor, pol, spot, inv_curv,
f, mode), make_beam's leading arguments."""
make_beams(p::GPUPlasma, launchers, s_max::Float64, psi_dP_dV::Vector{Float64}; kw...) =
    _make_beams(p, nothing, nothing, launchers, s_max, psi_dP_dV; kw...)

# the body of both make_beams methods: `plasmas === nothing` is the launching plasma for every beam
function _make_beams(p::GPUPlasma, plasmas, beam_plasma, launchers, s_max::Float64,
                     psi_dP_dV::Vector{Float64};
                     ds::Float64=1e-4, N_rings::Integer=3, min_azimuthal_points::Integer=5,
                     normalize_weight_sum::Bool=true, deposition::Integer=1, absorption::Integer=1,
                     traj_stride::Integer=1)
    traj_stride >= 1 || throw(ArgumentError("traj_stride must be >= 1"))
    B = length(launchers)
    beam_off, omega, mode = zeros(Cint, B + 1), zeros(B), zeros(Cint, B)
    fans = Vector{NTuple{3,Array{Float64}}}()
    for (b, (r, phi, z, tor, pol, spot, inv_curv, f, m)) in enumerate(launchers)
        pos, dirs, w = _launch_fan(r, phi, z, tor, pol, spot, inv_curv, f, N_rings, min_azimuthal_points,
                                   normalize_weight_sum)
        nr = length(w)
        push!(fans, (pos, dirs, w))
        beam_off[b + 1] = beam_off[b] + nr
        omega[b], mode[b] = 2π * f, m
    end
    pos, dirs, w = vcat((a[1] for a in fans)...), vcat((a[2] for a in fans)...), vcat((a[3] for a in fans)...)
    sel = plasmas === nothing ? () : (plasmas, Cint.(beam_plasma .- 1))  # the C tables count from 0
    xp, Np, s0, st = ray_entry_beams(p, sel..., beam_off, omega, mode, pos, dirs)
    for b in 1:B
        bad = count(st[beam_off[b]+1:beam_off[b+1]] .!= 0)
        bad == 0 || throw(AssertionError("beam $b: ray entry failed for $bad rays"))
    end
    n_steps = max(1, round(Int, s_max / ds))
    cfg = TraceCfg(omega[1], mode[1], ds, n_steps, max(1, n_steps ÷ 100), 1.0, 1e-6, absorption,
                   traj_stride, deposition, 0, 1e-6, 1e-6, s_max, 100)
    state, status, steps, dP, Pdep, traj = trace_beams(p, sel..., cfg, beam_off, omega, mode, xp, Np, w,
                                                        psi_dP_dV, pos, s0)
    # the shells' volumes: the launching plasma's, or each listed plasma's own
    dV = plasmas === nothing ? [shell_volumes(p, psi_dP_dV)] : [shell_volumes(q, psi_dP_dV) for q in plasmas]
    out = []
    for b in 1:B
        dP_dV = zeros(length(psi_dP_dV))
        dP_dV[1:end-1] .= dP[1:end-2, b] ./ dV[plasmas === nothing ? 1 : beam_plasma[b]]
        arc_lengths, trajectories, ray_powers = Vector{Vector{Float64}}(), Vector{Vector{Vector{Float64}}}(), Vector{Vector{Float64}}()
        for i in beam_off[b]+1:beam_off[b+1]
            k = steps[i] ÷ traj_stride
            s_i, x_i, τ_i = traj[i, 5, 1:k], [traj[i, 1:3, j] for j in 1:k], traj[i, 4, 1:k]
            if steps[i] % traj_stride != 0  # the final state is not a saved sample
                push!(s_i, fma(Float64(steps[i]), ds, s0[i])); push!(x_i, state[i, 1:3]); push!(τ_i, state[i, 7])
            end
            push!(arc_lengths, vcat(0.0, s0[i], s_i))
            push!(trajectories, vcat([pos[i, :]], [xp[i, :]], x_i))
            push!(ray_powers, vcat(1.0, 1.0, exp.(-τ_i)))
        end
        push!(out, (arc_lengths, trajectories, ray_powers, dP_dV, dP[end, b], w[beam_off[b]+1:beam_off[b+1]]))
    end
    return out
end
make_beams(p::TorJ.Plasma, args...; kw...) = make_beams(gpu_plasma(p), args...; kw...)

# ---- ... through differing plasmas (torj_trace_beams_plasmas) ----
# beam b goes through plasmas[beam_plasma[b]]; p is the launching handle (stream, scratch, knobs),
# listed or not; every listed plasma is on p's device.  The C tables count plasmas from 0.
_handles(plasmas::Vector{GPUPlasma}) = Ptr{Cvoid}[q.h for q in plasmas]

function ray_entry_beams(p::GPUPlasma, plasmas::Vector{GPUPlasma}, beam_plasma0::Vector{Cint},
                         beam_off::Vector{Cint}, omega::Vector{Float64}, mode::Vector{Cint},
                         x0::Matrix{Float64}, N0::Matrix{Float64})
    n = size(x0, 1)
    hs = _handles(plasmas)
    xp, Np, s0, st = zeros(n, 3), zeros(n, 3), zeros(n), zeros(Cint, n)
    GC.@preserve plasmas hs begin
        check(ccall((:torj_ray_entry_beams_plasmas_gpu, libtorj), Cint,
                    (Ptr{Cvoid}, Cint, Ptr{Ptr{Cvoid}}, Ptr{Cint}, Cint, Ptr{Cint}, Ptr{Float64}, Ptr{Cint},
                     Ptr{Float64}, Ptr{Float64}, Ptr{Float64}, Ptr{Float64}, Ptr{Float64}, Ptr{Cint}),
                    p.h, length(hs), hs, beam_plasma0, length(omega), beam_off, omega, mode, x0, N0, xp, Np,
                    s0, st))
    end
    return xp, Np, s0, st
end

function trace_beams(p::GPUPlasma, plasmas::Vector{GPUPlasma}, beam_plasma0::Vector{Cint}, cfg::TraceCfg,
                     beam_off::Vector{Cint}, omega::Vector{Float64}, mode::Vector{Cint},
                     x0::Matrix{Float64}, N0::Matrix{Float64}, w::Vector{Float64},
                     psi_grid::Vector{Float64}, x_launch::Matrix{Float64}, s0::Vector{Float64})
    n, B = size(x0, 1), length(omega)
    hs = _handles(plasmas)
    n_save = cfg.traj_stride > 0 ? cfg.n_steps ÷ cfg.traj_stride : 0
    state, status, steps = zeros(n, 7), zeros(Cint, n), zeros(Cint, n)
    dP, Pdep = zeros(length(psi_grid) + 1, B), zeros(n)
    traj = n_save > 0 ? zeros(n, 5, n_save) : zeros(0, 5, 0)
    GC.@preserve plasmas hs beam_plasma0 beam_off omega mode x0 N0 w psi_grid x_launch s0 begin
        check(ccall((:torj_trace_beams_plasmas, libtorj), Cint,
                    (Ptr{Cvoid}, Cint, Ptr{Ptr{Cvoid}}, Ptr{Cint}, Ref{TraceCfg}, Cint, Ptr{Cint}, Ptr{Float64},
                     Ptr{Cint}, Ptr{Float64}, Ptr{Float64}, Ptr{Float64}, Cint, Ptr{Float64}, Ptr{Float64},
                     Ptr{Float64}, Ptr{Float64}, Ptr{Cint}, Ptr{Cint}, Ptr{Float64}, Ptr{Float64}, Ptr{Float64}),
                    p.h, length(hs), hs, beam_plasma0, cfg, B, beam_off, omega, mode, x0, N0, w,
                    length(psi_grid), psi_grid, x_launch, s0, state, status, steps, dP, Pdep,
                    n_save > 0 ? traj : C_NULL))
    end
    return state, status, steps, dP, Pdep, traj
end

# ---- ray profiles (torj_ray_profile): N, the plasma parameters and alpha at every saved point ----
# the columns of a row, in the order of the header's TORJ_PROF_* enum
const PROFILE_COLUMNS = (:x, :y, :z, :Nx, :Ny, :Nz, :tau, :s, :P, :alpha, :dP_ds, :psi, :ne, :Te, :Bx, :By, :Bz,
                         :B_abs, :X, :Y, :N_par, :N_abs, :Ns2, :Lambda, :dLambda_dN)

"""ray_profile(p, cfg, beam_off, omega, mode, x0, N0; s0, plasmas, beam_plasma0) -- the rays of the
concatenated beams traced as trace_beams traces them without deposition; returns a NamedTuple of one
n x n_rows matrix per PROFILE_COLUMNS entry (row k: step (k - 1) * cfg.traj_stride, the first the entry
point; NaN where the ray had stopped) and `state`, `status`, `steps`.  A warm alpha along the ray:
alpha_warm's inputs are the columns X, Y, N_abs, N_par, Te and 1 ./ dLambda_dN."""
function ray_profile(p::GPUPlasma, cfg::TraceCfg, beam_off::Vector{Cint}, omega::Vector{Float64},
                     mode::Vector{Cint}, x0::Matrix{Float64}, N0::Matrix{Float64};
                     s0::Union{Nothing,Vector{Float64}}=nothing,
                     plasmas::Union{Nothing,Vector{GPUPlasma}}=nothing,
                     beam_plasma0::Union{Nothing,Vector{Cint}}=nothing)
    n = size(x0, 1)
    n_rows = cfg.traj_stride > 0 ? cfg.n_steps ÷ cfg.traj_stride + 1 : 0
    hs = plasmas === nothing ? Ptr{Cvoid}[] : _handles(plasmas)
    prof = zeros(n, length(PROFILE_COLUMNS), n_rows)
    state, status, steps = zeros(n, 7), zeros(Cint, n), zeros(Cint, n)
    GC.@preserve plasmas hs beam_plasma0 beam_off omega mode x0 N0 s0 begin
        check(ccall((:torj_ray_profile, libtorj), Cint,
                    (Ptr{Cvoid}, Cint, Ptr{Ptr{Cvoid}}, Ptr{Cint}, Ref{TraceCfg}, Cint, Ptr{Cint}, Ptr{Float64},
                     Ptr{Cint}, Ptr{Float64}, Ptr{Float64}, Ptr{Float64}, Cint, Ptr{Float64}, Ptr{Float64},
                     Ptr{Cint}, Ptr{Cint}),
                    p.h, length(hs), plasmas === nothing ? C_NULL : hs,
                    beam_plasma0 === nothing ? C_NULL : beam_plasma0, cfg, length(omega), beam_off, omega, mode,
                    x0, N0, s0 === nothing ? C_NULL : s0, n_rows, prof, state, status, steps))
    end
    cols = NamedTuple{PROFILE_COLUMNS}(ntuple(c -> prof[:, c, :], length(PROFILE_COLUMNS)))
    return merge(cols, (state=state, status=status, steps=steps))
end

# the device forms: every array but the five host tables is device memory (Ptr{Cvoid}), the call is
# enqueued on `stream`; torj_trace_check(p, stream) follows the last of them
function ray_entry_beams_device(p::GPUPlasma, plasmas::Vector{GPUPlasma}, beam_plasma0::Vector{Cint},
                                beam_off::Vector{Cint}, omega::Vector{Float64}, mode::Vector{Cint},
                                x0::Ptr{Cvoid}, N0::Ptr{Cvoid}, xp::Ptr{Cvoid}, Np::Ptr{Cvoid},
                                s0::Ptr{Cvoid}, status::Ptr{Cvoid}, stream::Ptr{Cvoid})
    hs = _handles(plasmas)
    GC.@preserve plasmas hs begin
        check(ccall((:torj_ray_entry_beams_plasmas_device, libtorj), Cint,
                    (Ptr{Cvoid}, Cint, Ptr{Ptr{Cvoid}}, Ptr{Cint}, Cint, Ptr{Cint}, Ptr{Float64}, Ptr{Cint},
                     Ptr{Float64}, Ptr{Float64}, Ptr{Float64}, Ptr{Float64}, Ptr{Float64}, Ptr{Cint},
                     Ptr{Cvoid}),
                    p.h, length(hs), hs, beam_plasma0, length(omega), beam_off, omega, mode,
                    Ptr{Float64}(x0), Ptr{Float64}(N0), Ptr{Float64}(xp), Ptr{Float64}(Np), Ptr{Float64}(s0),
                    Ptr{Cint}(status), stream))
    end
    return nothing
end

function trace_beams_device(p::GPUPlasma, plasmas::Vector{GPUPlasma}, beam_plasma0::Vector{Cint},
                            cfg::TraceCfg, beam_off::Vector{Cint}, omega::Vector{Float64},
                            mode::Vector{Cint}, x0::Ptr{Cvoid}, N0::Ptr{Cvoid}, w::Ptr{Cvoid}, n_psi::Integer,
                            psi_grid::Ptr{Cvoid}, x_launch::Ptr{Cvoid}, s0::Ptr{Cvoid}, state::Ptr{Cvoid},
                            status::Ptr{Cvoid}, steps::Ptr{Cvoid}, dP::Ptr{Cvoid}, Pdep::Ptr{Cvoid},
                            traj::Ptr{Cvoid}, counters::Ptr{Cvoid}, stream::Ptr{Cvoid})
    hs = _handles(plasmas)
    GC.@preserve plasmas hs begin
        check(ccall((:torj_trace_beams_plasmas_device, libtorj), Cint,
                    (Ptr{Cvoid}, Cint, Ptr{Ptr{Cvoid}}, Ptr{Cint}, Ref{TraceCfg}, Cint, Ptr{Cint}, Ptr{Float64},
                     Ptr{Cint}, Ptr{Float64}, Ptr{Float64}, Ptr{Float64}, Cint, Ptr{Float64}, Ptr{Float64},
                     Ptr{Float64}, Ptr{Float64}, Ptr{Cint}, Ptr{Cint}, Ptr{Float64}, Ptr{Float64}, Ptr{Float64},
                     Ptr{UInt64}, Ptr{Cvoid}),
                    p.h, length(hs), hs, beam_plasma0, cfg, length(omega), beam_off, omega, mode,
                    Ptr{Float64}(x0), Ptr{Float64}(N0), Ptr{Float64}(w), n_psi, Ptr{Float64}(psi_grid),
                    Ptr{Float64}(x_launch), Ptr{Float64}(s0), Ptr{Float64}(state), Ptr{Cint}(status),
                    Ptr{Cint}(steps), Ptr{Float64}(dP), Ptr{Float64}(Pdep), Ptr{Float64}(traj),
                    Ptr{UInt64}(counters), stream))
    end
    return nothing
end

"""make_beams(p, plasmas, beam_plasma, launchers, s_max, psi_dP_dV; ...) -- launcher b through
plasmas[beam_plasma[b]] (indices from 1), all in ONE launch on p's device; tuple b equals
make_beam's on that plasma, dP_dV taken with that plasma's shell volumes."""
function make_beams(p::GPUPlasma, plasmas::Vector{GPUPlasma}, beam_plasma::Vector{<:Integer}, launchers,
                    s_max::Float64, psi_dP_dV::Vector{Float64}; kw...)
    length(beam_plasma) == length(launchers) || throw(ArgumentError("beam_plasma needs one entry per launcher"))
    all(1 .<= beam_plasma .<= length(plasmas)) || throw(ArgumentError("beam_plasma must index plasmas (from 1)"))
    return _make_beams(p, plasmas, beam_plasma, launchers, s_max, psi_dP_dV; kw...)
end

# ---- make_beams as one C call (torj_make_beams): a ray that fails entry is reported, not fatal ----
struct Launcher              # torj_launcher
    r::Float64
    phi::Float64
    z::Float64
    steering_angle_tor::Float64
    steering_angle_pol::Float64
    spot_size::Float64
    inverse_curvature_radius::Float64
    f::Float64
    mode::Cint
    plasma::Cint             # from 0: the C table's index
end

struct BeamResult            # torj_beam_result
    n_rays::Cint
    n_ok::Cint
    first_bad_ray::Cint      # from 0 within the beam; -1 when every ray entered
    first_bad_status::Cint
    w_ok::Float64
    deposited_power::Float64
end

struct BeamsRays             # torj_beams_rays
    pos::Ptr{Float64}
    dir::Ptr{Float64}
    weights::Ptr{Float64}
    x_plasma::Ptr{Float64}
    N_plasma::Ptr{Float64}
    s0::Ptr{Float64}
    entry_status::Ptr{Cint}
    state::Ptr{Float64}
    status::Ptr{Cint}
    steps::Ptr{Cint}
    P_dep::Ptr{Float64}
    traj::Ptr{Float64}
end

# The one call.  Its three struct pointers are typed here (Ptr{Launcher}, Ptr{BeamResult},
# Ptr{BeamsRays}) and written with the @ccall macro; tests/test_make_beams_shim.py checks the
# call and the three structs against the header, field by field and argument by argument.
# `rays` is C_NULL (the count-only call: a Ptr argument may be NULL, a Ref one may not) or a
# Ref{BeamsRays}, which the call converts to the pointer and keeps alive.
function _torj_make_beams(p::GPUPlasma, hs, la::Vector{Launcher}, N_rings::Integer, min_az::Integer, cfg,
                          psi_dP_dV, dP_dV, res, off::Vector{Cint}, rays)
    return @ccall libtorj.torj_make_beams(p.h::Ptr{Cvoid}, (hs === C_NULL ? 0 : length(hs))::Cint,
                                          hs::Ptr{Ptr{Cvoid}}, length(la)::Cint, la::Ptr{Launcher},
                                          N_rings::Cint, min_az::Cint, cfg::Ref{TraceCfg},
                                          length(psi_dP_dV)::Cint, psi_dP_dV::Ptr{Float64},
                                          dP_dV::Ptr{Float64}, res::Ptr{BeamResult}, off::Ptr{Cint},
                                          rays::Ptr{BeamsRays})::Cint
end

"""make_beams_c(p, launchers, s_max, psi_dP_dV; plasmas, beam_plasma, ...) -> (tuples, results):
make_beams through the one C entry point.  A ray that fails entry does not throw: results[b]
(a BeamResult) says how many of beam b's rays entered, which failed first and how much of the
launched weight coupled, and the per-ray lists of tuples[b] are over the rays that entered, with
their launched weights.  `beam_plasma` indexes `plasmas` from 1."""
function make_beams_c(p::GPUPlasma, launchers, s_max::Float64, psi_dP_dV::Vector{Float64};
                      plasmas::Union{Nothing,Vector{GPUPlasma}}=nothing,
                      beam_plasma::Union{Nothing,Vector{<:Integer}}=nothing, ds::Float64=1e-4,
                      N_rings::Integer=3, min_azimuthal_points::Integer=5, deposition::Integer=1,
                      absorption::Integer=1, traj_stride::Integer=1)
    traj_stride >= 1 || throw(ArgumentError("traj_stride must be >= 1"))
    (plasmas === nothing) == (beam_plasma === nothing) || throw(ArgumentError("plasmas and beam_plasma go together"))
    B = length(launchers)
    beam_plasma === nothing || length(beam_plasma) == B || throw(ArgumentError("beam_plasma needs one entry per launcher"))
    la = [Launcher(l[1], l[2], l[3], l[4], l[5], l[6], l[7], l[8], l[9],
                   beam_plasma === nothing ? 0 : beam_plasma[b] - 1) for (b, l) in enumerate(launchers)]
    hs = plasmas === nothing ? C_NULL : _handles(plasmas)
    n_steps = max(1, round(Int, s_max / ds))
    cfg = TraceCfg(0.0, 0, ds, n_steps, max(1, n_steps ÷ 100), 1.0, 1e-6, absorption, traj_stride, deposition,
                   0, 1e-6, 1e-6, s_max, 100)
    off = zeros(Cint, B + 1)
    n_psi = length(psi_dP_dV)
    GC.@preserve plasmas hs begin
        check(_torj_make_beams(p, hs, la, N_rings, min_azimuthal_points, cfg, psi_dP_dV, C_NULL, C_NULL, off,
                               C_NULL))  # the ray count
        n, n_save = Int(off[end]), n_steps ÷ traj_stride
        pos, dirs, w = zeros(n, 3), zeros(n, 3), zeros(n)
        xp, Np, s0, est = zeros(n, 3), zeros(n, 3), zeros(n), zeros(Cint, n)
        state, status, steps, Pdep = zeros(n, 7), zeros(Cint, n), zeros(Cint, n), zeros(n)
        traj = zeros(n, 5, n_save)
        dP_dV, res = zeros(n_psi, B), Vector{BeamResult}(undef, B)
        GC.@preserve pos dirs w xp Np s0 est state status steps Pdep traj begin
            rays = BeamsRays(pointer(pos), pointer(dirs), pointer(w), pointer(xp), pointer(Np), pointer(s0),
                             pointer(est), pointer(state), pointer(status), pointer(steps), pointer(Pdep),
                             n_save > 0 ? pointer(traj) : Ptr{Float64}(C_NULL))
            check(_torj_make_beams(p, hs, la, N_rings, min_azimuthal_points, cfg, psi_dP_dV, dP_dV, res, off,
                                   Ref(rays)))
        end
    end
    tuples = []
    for b in 1:B
        arc_lengths, trajectories, ray_powers = Vector{Vector{Float64}}(), Vector{Vector{Vector{Float64}}}(), Vector{Vector{Float64}}()
        ok = [i for i in off[b]+1:off[b+1] if est[i] == 0]
        for i in ok
            k = steps[i] ÷ traj_stride
            s_i, x_i, τ_i = traj[i, 5, 1:k], [traj[i, 1:3, j] for j in 1:k], traj[i, 4, 1:k]
            if steps[i] % traj_stride != 0  # the final state is not a saved sample
                push!(s_i, fma(Float64(steps[i]), ds, s0[i])); push!(x_i, state[i, 1:3]); push!(τ_i, state[i, 7])
            end
            push!(arc_lengths, vcat(0.0, s0[i], s_i))
            push!(trajectories, vcat([pos[i, :]], [xp[i, :]], x_i))
            push!(ray_powers, vcat(1.0, 1.0, exp.(-τ_i)))
        end
        push!(tuples, (arc_lengths, trajectories, ray_powers, dP_dV[:, b], res[b].deposited_power, w[ok]))
    end
    return tuples, res
end
make_beams_c(p::TorJ.Plasma, args...; kw...) = make_beams_c(gpu_plasma(p), args...; kw...)

"""alpha(...) of src/general_absorption.jl:1328-1337 (repaired, DESIGN.md §3.6) at n
points on the GPU: iwarm 1 (weakly) or 3 (fully relativistic); inv_dDdN = 1/|dD/dN|.
Returns (alpha, N_perp^2)."""
function alpha_warm(omega::Vector{Float64}, X::Vector{Float64}, Y::Vector{Float64},
                    N_abs::Vector{Float64}, N_par::Vector{Float64}, Te::Vector{Float64},
                    inv_dDdN::Vector{Float64}, mode::Integer, iwarm::Integer)
    n = length(X)
    alpha, n2 = zeros(n), zeros(2n)
    check(ccall((:torj_alpha_warm, libtorj), Cint,
                (Cint, Ptr{Float64}, Ptr{Float64}, Ptr{Float64}, Ptr{Float64}, Ptr{Float64},
                 Ptr{Float64}, Ptr{Float64}, Cint, Cint, Ptr{Float64}, Ptr{Float64}),
                n, omega, X, Y, N_abs, N_par, Te, inv_dDdN, mode, iwarm, alpha, n2))
    return alpha, complex.(n2[1:2:end], n2[2:2:end])
end

end # module
