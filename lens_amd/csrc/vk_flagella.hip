// Motile agents with a multi-flagellar motor on MI355X (gfx950): the chemoreceptor cluster,
// FlagellaActivity and a run-and-tumble move, one thread per agent, `substeps` inner updates
// per call.  Sense, receptor and move are the coarse kernel's (vk_motile.h); the motor is
//   FlagellaActivity.next_update   vivarium/processes/flagella_activity.py:135-261
// (Mears et al. 2014, Sneddon et al. 2012), restated in its operation order and compiled with
// -ffp-contract=off.  One inner update of h seconds:
//   1. count change: new = target - have, decided now, applied after step 4 (a flagellum
//      removed in an update still switches and still counts in it, one added does neither);
//   2. CheY-P, an Ornstein-Uhlenbeck step: dYP = -(1/tau) (CheY_P - YP_ss) h + amp z with
//      amp = sqrt(sigma2_Y) sqrt(2 h / tau) (the reference writes x**0.5; amp is evaluated once
//      per launch on the host with the correctly rounded sqrt), CheY_P = max(CheY_P + dYP, 0),
//      CheY = max(CheY - dYP, 0);
//   3. every existing flagellum switches with probability rate * h, the rates from the
//      updated CheY_P: CW->CCW omega exp(dg), CCW->CW omega exp(-dg);
//   4. motile state: tumble (1) if any flagellum is CW, else run (-1) if there was a
//      flagellum or one was added, else none (0); thrust = scaling PMF flagellum_thrust target.
// As in the reference the receptor's activity does not reach this motor.  cw_bias is emitted
// and read by nothing, so it is evaluated once, from the CheY_P of the last inner update.
//
// The flagella of an agent are one 32-bit mask (bit i set: flagellum i turns CW; bits at and
// above `have` are zero), so the loop over them has a per-lane trip count and indexes nothing.
// Removing flagellum j deletes bit j and closes the gap; new flagella go above `have`.
//
// NOT reference parity, as in the coarse kernel: the kinematics (speed = run_speed * thrust /
// 250 along the heading, a Gaussian heading change while tumbling, reflecting walls; torque is
// the heading change / h, not the reference's tumble_jitter draw), and target is clamped to 32.
//
// Random numbers: philox_uniform(seed, s, k, 0, path) at global inner update s for the agent
// with key k -- independent of storage order, launch geometry and graph replay.  Paths:
//   1, 2      the tumble heading's Box-Muller pair (as in the coarse kernel; 0 is its switch)
//   3, 4      the CheY-P Box-Muller pair
//   16 + i    flagellum i's switch, i < 32
//   64 + r    the r-th structural draw of the update, r < 32: a removal index
//             j = floor(u * remaining), or a new flagellum's state (CW when u < 0.5)

#include "vk_motile.h"

template <class Sense>
__global__ __launch_bounds__(256) void k_flagella_step(
    vk_motility_params p, vk_flagella_params f, int64_t n, int64_t ld, double h, double amp, int substeps,
    double *__restrict__ motil, double *__restrict__ flag, int32_t *__restrict__ flag_int, double *__restrict__ loc,
    const int64_t *__restrict__ key, Sense sense, int nx, int ny, double bx, double by,
    double bx_below, double by_below, const uint64_t *__restrict__ counter, int32_t *__restrict__ bin_lin,
    int32_t *__restrict__ ix_out) {
    const int64_t a = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (a >= n) return;
    const int32_t k = key ? (int32_t)key[a] : (int32_t)a;
    const uint64_t s0 = counter[0];
    double n_methyl = motil[(int64_t)VK_MOTIL_N_METHYL * ld + a];
    double P_on = motil[(int64_t)VK_MOTIL_ACTIVITY * ld + a];
    double angle = motil[(int64_t)VK_MOTIL_ANGLE * ld + a];
    double CheY = flag[(int64_t)VK_FLAG_CHEY * ld + a];
    double CheY_P = flag[(int64_t)VK_FLAG_CHEY_P * ld + a];
    const double PMF = flag[(int64_t)VK_FLAG_PMF * ld + a];
    const int target = min(max(flag_int[(int64_t)VK_FLAGI_TARGET * ld + a], 0), 32);
    int have = min(max(flag_int[(int64_t)VK_FLAGI_HAVE * ld + a], 0), 32);
    uint32_t mask = (uint32_t)flag_int[(int64_t)VK_FLAGI_MASK * ld + a];
    if (have < 32) mask &= (1u << have) - 1u;
    double x = loc[a], y = loc[ld + a];
    int ix;
    int32_t bin = bin_site_lin(x, y, nx, ny, bx, by, 0, &ix);
    const double CheR = p.CheR * 1e3, CheB = p.CheB * 1e3;
    int motile = 0;
    double thrust = 0.0, torque = 0.0;
    for (int s = 0; s < substeps; ++s) {
        // (a) sense, (b) receptor: the coarse kernel's
        const double L = motile_sense(sense, bin, x, y);
        motile_receptor(p, CheR, CheB, L, h, n_methyl, P_on);
        const uint64_t step = s0 + (uint64_t)s;

        // (c) 2. CheY-P
        const double dYP = -(1.0 / f.tau) * (CheY_P - f.YP_ss) * h + amp * motile_normal(p.seed, step, k, 3);
        CheY_P = fmax(CheY_P + dYP, 0.0);
        CheY = fmax(CheY - dYP, 0.0);

        // 3. the existing flagella, from the updated CheY_P
        const double delta_g = f.g_0 / 4.0 - f.g_1 / 2.0 * (CheY_P / (CheY_P + f.K_D));
        const double p_cw = f.omega * exp(delta_g) * h;       // CW -> CCW
        const double p_ccw = f.omega * exp(-delta_g) * h;     // CCW -> CW
        for (int i = 0; i < have; ++i) {
            const double u = philox_uniform(p.seed, step, k, 0, 16 + i);
            if (u <= ((mask >> i) & 1u ? p_cw : p_ccw)) mask ^= 1u << i;
        }

        // 4. motile state and thrust, from the flagella of step 3 and the target count
        const int change = target - have;
        if (mask != 0u) {
            motile = 1;
            thrust = f.tumble_scaling * PMF * f.flagellum_thrust * (double)target;
        } else if (have > 0 || change > 0) {
            motile = -1;
            thrust = f.run_scaling * PMF * f.flagellum_thrust * (double)target;
        } else {
            motile = 0;
            thrust = 0.0;
        }

        // 1. the count change takes effect
        if (change < 0) {
            for (int r = 0; r < -change; ++r) {
                const int remaining = have - r;
                const double u = philox_uniform(p.seed, step, k, 0, 64 + r);
                const int j = min((int)(u * (double)remaining), remaining - 1);
                mask = (mask & ((1u << j) - 1u)) | (((mask >> j) >> 1) << j);
            }
        } else {
            for (int r = 0; r < change; ++r)
                if (philox_uniform(p.seed, step, k, 0, 64 + r) < 0.5) mask |= 1u << (have + r);
        }
        have = target;

        // (d) kinematics: this engine's stand-in for the reference's pymunk multibody
        torque = 0.0;
        if (motile == 1) torque = motile_tumble(p, step, k, h, angle);
        const double speed = p.run_speed * thrust / 250.0;
        bin = motile_move(speed, h, angle, x, y, nx, ny, bx, by, bx_below, by_below, &ix);
    }
    const double yh = pow(CheY_P, f.H);
    motil[(int64_t)VK_MOTIL_N_METHYL * ld + a] = n_methyl;
    motil[(int64_t)VK_MOTIL_ACTIVITY * ld + a] = P_on;
    motil[(int64_t)VK_MOTIL_MOTOR_STATE * ld + a] = motile == 1 ? 1.0 : 0.0;
    motil[(int64_t)VK_MOTIL_ANGLE * ld + a] = angle;
    motil[(int64_t)VK_MOTIL_THRUST * ld + a] = thrust;
    motil[(int64_t)VK_MOTIL_TORQUE * ld + a] = torque;
    flag[(int64_t)VK_FLAG_CHEY * ld + a] = CheY;
    flag[(int64_t)VK_FLAG_CHEY_P * ld + a] = CheY_P;
    flag[(int64_t)VK_FLAG_CW_BIAS * ld + a] = yh / (pow(f.K_d, f.H) + yh);
    flag[(int64_t)VK_FLAG_MOTILE_STATE * ld + a] = (double)motile;
    flag_int[(int64_t)VK_FLAGI_HAVE * ld + a] = have;
    flag_int[(int64_t)VK_FLAGI_MASK * ld + a] = (int32_t)mask;
    loc[a] = x;
    loc[ld + a] = y;
    bin_lin[a] = bin;
    if (ix_out) ix_out[a] = ix;
}

// the launch both entry points share: the agents' kernel, then the counter
template <class Sense>
static int flagella_launch(const char *what, const vk_motility_params *p, const vk_flagella_params *f, int64_t n,
                           int64_t ld, double dt, int32_t substeps, double *motil, double *flag, int32_t *flag_int,
                           double *loc, const int64_t *key, const Sense &sense, int32_t nx, int32_t ny, double bound_x,
                           double bound_y, uint64_t *counter, int32_t *bin_lin, int32_t *ix_out, vk_stream_t stream) {
    if (!p || !f || n < 0 || ld < n || substeps < 1 || !(dt > 0.0) || nx <= 0 || ny <= 0 || !(bound_x > 0.0) ||
        !(bound_y > 0.0) || (int64_t)nx * ny >= INT32_MAX || !counter || !(f->tau > 0.0) || !(f->sigma2_Y >= 0.0) ||
        (n > 0 && (!motil || !flag || !flag_int || !loc || !bin_lin))) {
        vk::set_error("%s: bad arguments", what);
        return VK_ERR_ARG;
    }
    hipStream_t s = (hipStream_t)stream;
    if (n > 0) {
        const double h = dt / substeps;
        const double amp = sqrt(f->sigma2_Y) * sqrt(2.0 * h / f->tau);
        hipLaunchKernelGGL(k_flagella_step<Sense>, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, s, *p, *f, n, ld,
                           h, amp, substeps, motil, flag, flag_int, loc, key, sense, nx, ny, bound_x, bound_y,
                           nextafter(bound_x, 0.0), nextafter(bound_y, 0.0), counter, bin_lin, ix_out);
        const int rc = vk::launch_check("k_flagella_step");
        if (rc) return rc;
    }
    // the counter advances for an empty colony too: s counts inner updates, not agents
    hipLaunchKernelGGL(k_motile_advance, dim3(1), dim3(64), 0, s, counter, (uint64_t)substeps);
    return vk::launch_check("k_motile_advance");
}

extern "C" int vk_flagella_step(const vk_motility_params *p, const vk_flagella_params *f, int64_t n, int64_t ld,
                                double dt, int32_t substeps, double *motil, double *flag, int32_t *flag_int,
                                double *loc, const int64_t *key, const double *ligand, int32_t nx, int32_t ny,
                                double bound_x, double bound_y, uint64_t *counter, int32_t *bin_lin, int32_t *ix_out,
                                vk_stream_t stream) {
    if (n > 0 && !ligand) {
        vk::set_error("vk_flagella_step: bad arguments");
        return VK_ERR_ARG;
    }
    return flagella_launch<sense_plane>("vk_flagella_step", p, f, n, ld, dt, substeps, motil, flag, flag_int, loc, key,
                           sense_plane(ligand), nx, ny, bound_x, bound_y, counter, bin_lin, ix_out, stream);
}

extern "C" int vk_flagella_step_static(const vk_motility_params *p, const vk_flagella_params *f, int64_t n,
                                       int64_t ld, double dt, int32_t substeps, double *motil, double *flag,
                                       int32_t *flag_int, double *loc, const int64_t *key,
                                       const vk_gradient_spec *ligand, int32_t nx, int32_t ny, double bound_x,
                                       double bound_y, uint64_t *counter, int32_t *bin_lin, int32_t *ix_out,
                                       vk_stream_t stream) {
    if (!ligand || !gradient_spec_ok(*ligand)) {
        vk::set_error("vk_flagella_step_static: bad arguments");
        return VK_ERR_ARG;
    }
    return flagella_launch<sense_static>("vk_flagella_step_static", p, f, n, ld, dt, substeps, motil, flag, flag_int, loc, key,
                           *ligand, nx, ny, bound_x, bound_y, counter, bin_lin, ix_out, stream);
}
