// Motile agents on MI355X (gfx950): chemoreceptor cluster, flagellar motor and a
// run-and-tumble move, one thread per agent, `substeps` inner updates per call.
//
// Reference semantics, restated in the reference's operation order (compiled with
// -ffp-contract=off, so the +, -, x, / sequences round as the reference's Python does;
// log / exp / sin / cos are the device library's, within an ulp or two of libm's):
//   ReceptorCluster.next_update   vivarium/processes/chemoreceptor_cluster.py:166-209
//   MotorActivity.next_update     vivarium/processes/coarse_motor.py:134-164 (+ run / tumble :177-190)
// The reference converts CheR / CheB from mM to uM through pint
// (`.to('umol/L').magnitude`).  pint was not available when this was written, so the factor
// is taken as x * 1e3 and is NOT pinned against the reference's units library.
// Where the reference's motor raises a math domain error (a switching rate r >= 1 makes
// log(1 - r) undefined) the switch probability here is 1.
//
// NOT reference parity: the kinematics.  The reference hands thrust and torque to a pymunk
// rigid-body simulation (multibody); this engine has no multibody physics, and moves each
// agent with its own stand-in: a constant run speed along the heading, a slower drift and a
// Gaussian heading change while tumbling, reflecting walls.  thrust / torque are still
// emitted (250 / 0 running, 100 / d(angle)/dt tumbling); the speed is run_speed * thrust / 250.
// Receptor, tumble and move are shared with the flagella kernel (vk_motile.h).
//
// Random numbers: draw j in {0, 1, 2} of the agent with reference-order key k at global
// inner update s is philox_uniform(seed, s, k, 0, j) -- independent of storage order and
// launch geometry.  s comes from a one-element device counter that the launch sequence
// advances by `substeps`, so a captured graph replays successive steps.
//
// A streaming kernel: per agent it reads and writes 9 state rows and the location once, and
// reads one ligand value per inner update; the state of an agent lives in registers between.
// vk_motility_step_static is the same kernel body with the sensing swapped (vk_motile.h): the
// ligand is an analytic gradient evaluated at the agent's position, nothing is read per update.

#include "vk_motile.h"

template <class Sense>
__global__ __launch_bounds__(256) void k_motility_step(vk_motility_params p, int64_t n, int64_t ld, double h,
                                                       int substeps, double *__restrict__ motil,
                                                       double *__restrict__ loc, const int64_t *__restrict__ key,
                                                       Sense sense, int nx, int ny, double bx,
                                                       double by, double bx_below, double by_below,
                                                       const uint64_t *__restrict__ counter,
                                                       int32_t *__restrict__ bin_lin, int32_t *__restrict__ ix_out) {
    const int64_t a = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (a >= n) return;
    const int32_t k = key ? (int32_t)key[a] : (int32_t)a;
    const uint64_t s0 = counter[0];
    double n_methyl = motil[(int64_t)VK_MOTIL_N_METHYL * ld + a];
    double P_on = motil[(int64_t)VK_MOTIL_ACTIVITY * ld + a];
    double CheY_P = motil[(int64_t)VK_MOTIL_CHEY_P * ld + a];
    double ccw_motor_bias = motil[(int64_t)VK_MOTIL_CCW_MOTOR_BIAS * ld + a];
    double ccw_to_cw = motil[(int64_t)VK_MOTIL_CCW_TO_CW * ld + a];
    bool tumbling = motil[(int64_t)VK_MOTIL_MOTOR_STATE * ld + a] != 0.0;
    double angle = motil[(int64_t)VK_MOTIL_ANGLE * ld + a];
    double thrust = motil[(int64_t)VK_MOTIL_THRUST * ld + a];
    double torque = motil[(int64_t)VK_MOTIL_TORQUE * ld + a];
    double x = loc[a], y = loc[ld + a];
    int ix;
    int32_t bin = bin_site_lin(x, y, nx, ny, bx, by, 0, &ix);
    // mM -> uM (see the header: the reference's pint conversion, unpinned)
    const double CheR = p.CheR * 1e3, CheB = p.CheB * 1e3;
    for (int s = 0; s < substeps; ++s) {
        // (a) sense (vk_motile.h): a plane is not written here, so this is the pre-step field; an
        // analytic field is read where the previous inner update left the agent
        const double L = motile_sense(sense, bin, x, y);

        // (b) receptor (vk_motile.h; the clamp quirk is kept there)
        motile_receptor(p, CheR, CheB, L, h, n_methyl, P_on);

        // (c) motor, from the activity just computed
        CheY_P = p.adapt_precision * p.k_y * p.k_s * P_on / (p.k_y * p.k_s * P_on + p.k_z + p.gamma_Y);
        ccw_motor_bias = p.mb_0 / (CheY_P * (1.0 - p.mb_0) + p.mb_0);
        ccw_to_cw = p.cw_to_ccw * (1.0 / ccw_motor_bias - 1.0);
        if (ccw_to_cw < p.cw_to_ccw_leak) ccw_to_cw = p.cw_to_ccw_leak;
        const double r = tumbling ? p.cw_to_ccw : ccw_to_cw;
        double prob_switch = 1.0;
        if (r < 1.0) {
            const double rate = -log(1.0 - r);
            prob_switch = 1.0 - exp(-rate * h);
        }
        const uint64_t step = s0 + (uint64_t)s;
        if (philox_uniform(p.seed, step, k, 0, 0) <= prob_switch) tumbling = !tumbling;

        // (d) kinematics: this engine's stand-in for the reference's pymunk multibody
        double speed;
        if (tumbling) {
            torque = motile_tumble(p, step, k, h, angle);
            speed = p.run_speed * 100.0 / 250.0;
            thrust = 100.0;
        } else {
            speed = p.run_speed;
            thrust = 250.0;
            torque = 0.0;
        }
        bin = motile_move(speed, h, angle, x, y, nx, ny, bx, by, bx_below, by_below, &ix);
    }
    motil[(int64_t)VK_MOTIL_N_METHYL * ld + a] = n_methyl;
    motil[(int64_t)VK_MOTIL_ACTIVITY * ld + a] = P_on;
    motil[(int64_t)VK_MOTIL_CHEY_P * ld + a] = CheY_P;
    motil[(int64_t)VK_MOTIL_CCW_MOTOR_BIAS * ld + a] = ccw_motor_bias;
    motil[(int64_t)VK_MOTIL_CCW_TO_CW * ld + a] = ccw_to_cw;
    motil[(int64_t)VK_MOTIL_MOTOR_STATE * ld + a] = tumbling ? 1.0 : 0.0;
    motil[(int64_t)VK_MOTIL_ANGLE * ld + a] = angle;
    motil[(int64_t)VK_MOTIL_THRUST * ld + a] = thrust;
    motil[(int64_t)VK_MOTIL_TORQUE * ld + a] = torque;
    loc[a] = x;
    loc[ld + a] = y;
    bin_lin[a] = bin;
    if (ix_out) ix_out[a] = ix;
}

// the launch both entry points share: the agents' kernel, then the counter
template <class Sense>
static int motility_launch(const char *what, const vk_motility_params *p, int64_t n, int64_t ld, double dt,
                           int32_t substeps, double *motil, double *loc, const int64_t *key, const Sense &sense,
                           int32_t nx, int32_t ny, double bound_x, double bound_y, uint64_t *counter,
                           int32_t *bin_lin, int32_t *ix_out, vk_stream_t stream) {
    if (!p || n < 0 || ld < n || substeps < 1 || !(dt > 0.0) || nx <= 0 || ny <= 0 || !(bound_x > 0.0) ||
        !(bound_y > 0.0) || (int64_t)nx * ny >= INT32_MAX || !counter || (n > 0 && (!motil || !loc || !bin_lin))) {
        vk::set_error("%s: bad arguments", what);
        return VK_ERR_ARG;
    }
    hipStream_t s = (hipStream_t)stream;
    if (n > 0) {
        hipLaunchKernelGGL(k_motility_step<Sense>, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, s, *p, n, ld,
                           dt / substeps, substeps, motil, loc, key, sense, nx, ny, bound_x, bound_y,
                           nextafter(bound_x, 0.0), nextafter(bound_y, 0.0), counter, bin_lin, ix_out);
        const int rc = vk::launch_check("k_motility_step");
        if (rc) return rc;
    }
    // the counter advances for an empty colony too: s counts inner updates, not agents
    hipLaunchKernelGGL(k_motile_advance, dim3(1), dim3(64), 0, s, counter, (uint64_t)substeps);
    return vk::launch_check("k_motile_advance");
}

extern "C" int vk_motility_step(const vk_motility_params *p, int64_t n, int64_t ld, double dt, int32_t substeps,
                                double *motil, double *loc, const int64_t *key, const double *ligand, int32_t nx,
                                int32_t ny, double bound_x, double bound_y, uint64_t *counter, int32_t *bin_lin,
                                int32_t *ix_out, vk_stream_t stream) {
    if (n > 0 && !ligand) {
        vk::set_error("vk_motility_step: bad arguments");
        return VK_ERR_ARG;
    }
    return motility_launch<sense_plane>("vk_motility_step", p, n, ld, dt, substeps, motil, loc, key, sense_plane(ligand), nx, ny,
                           bound_x, bound_y, counter, bin_lin, ix_out, stream);
}

extern "C" int vk_motility_step_static(const vk_motility_params *p, int64_t n, int64_t ld, double dt,
                                       int32_t substeps, double *motil, double *loc, const int64_t *key,
                                       const vk_gradient_spec *ligand, int32_t nx, int32_t ny, double bound_x,
                                       double bound_y, uint64_t *counter, int32_t *bin_lin, int32_t *ix_out,
                                       vk_stream_t stream) {
    if (!ligand || !gradient_spec_ok(*ligand)) {
        vk::set_error("vk_motility_step_static: bad arguments");
        return VK_ERR_ARG;
    }
    return motility_launch<sense_static>("vk_motility_step_static", p, n, ld, dt, substeps, motil, loc, key, *ligand,
                           nx, ny, bound_x, bound_y, counter, bin_lin, ix_out, stream);
}
