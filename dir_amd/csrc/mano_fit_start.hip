// dir_mano_fit_start: the closed-form start of a MANO fit -- p0's root (6 floats) and camera (3 floats) moved to where a rigid alignment, a
// search over the cube's 24 rotations and a least-squares camera put them; the other 55 floats copied.  The rule, the order of every sum and
// the status bits are written out in include/dir_hip.h ("MANO fitting: closed-form start"); tests/helpers/mano_start_ref.py restates it.
//
// One 256-thread workgroup per (sample, hand), as mano_fit_kernel.  The forward at p0 is mano_device.h's forward schedule, run ONCE, behind the
// target scan the fit kernels run (mano_fit_device.h); what follows is two
// reductions over the 778 vertices (the cross-covariance and the energy before; the energy after), one thread solving Horn's 4 x 4 eigenproblem
// (horn_rotation.h, the solver dir_procrustes_align runs), 24 threads fitting one camera each over 21 keypoints, and one thread deciding.
// fp32 throughout, every sum in a fixed order, no atomics, no workspace: a row gives the same bits in any slot of any batch and in either hand slot.
#include "horn_rotation.h"
#include "mano_fit_device.h"

namespace {

using namespace dir::mano;
using dir::finite;

constexpr int NRED = 11;                 // S [9] | e0 | W

struct StartArgs {
    dir_mano_tables t[2];
    dir_mano_fit_start_hand h[2];
    float kv, kj;                        // w_verts / 778, w_joints / 21: formed in double on the host, rounded once
    int root, cam, search;
};

// the joints that are rigid under the root (pd_joint_xyz_* order): wrist, thumb base, the four MCPs; the root_palm wrist is two skinned vertices
__device__ __forceinline__ bool rigid_joint(int j, int root_palm) { return (j == 0 && !root_palm) || j == 1 || j == 5 || j == 9 || j == 13 || j == 17; }

// candidate k of the 24 proper rotations of the cube: row r has sign sg[r] at column perm[r] (include/dir_hip.h gives the numbering)
__device__ __forceinline__ void cube_rotation(int k, int (&perm)[3], float (&sg)[3]) {
    const int pi = k >> 2, r = k & 3;
    const int p0 = pi >> 1, rest = pi & 1;                        // lexicographic: 012 021 102 120 201 210
    const int lo = p0 == 0 ? 1 : 0, hi = p0 == 2 ? 1 : 2;
    perm[0] = p0; perm[1] = rest ? hi : lo; perm[2] = rest ? lo : hi;
    const bool even = pi == 0 || pi == 3 || pi == 4;
    const int i = even ? (r == 0 ? 0 : r == 1 ? 3 : r == 2 ? 5 : 6) : (r == 0 ? 1 : r == 1 ? 2 : r == 2 ? 4 : 7);      // the sign triples with det +1
    sg[0] = (i & 4) ? -1.f : 1.f; sg[1] = (i & 2) ? -1.f : 1.f; sg[2] = (i & 1) ? -1.f : 1.f;
}

__global__ __launch_bounds__(BT) void mano_fit_start_kernel(StartArgs args) {
    const dir_mano_tables& T = args.t[blockIdx.y];
    const dir_mano_fit_start_hand& a = args.h[blockIdx.y];
    const int side = T.side, center = T.center_idx, root_palm = T.root_palm;       // read once, here (mano_device.h, layer 2)
    __shared__ float s_v[NV3P];          // v_posed
    __shared__ float s_vert[NV3P];       // skinned vertices (before centring)
    __shared__ float s_p[64];
    __shared__ float s_full[45];
    DIR_MANO_LDS(L, s);
    __shared__ float s_red[4][NRED], s_sum[NRED], s_e1[4];
    __shared__ float s_Q[9], s_pi[3], s_Y[63];       // Horn's rotation, the pivot, the joints under the root of step 2 (relative to the centre)
    __shared__ float s_cand[25][5];                  // per candidate: e_k, s, tx, ty, the residual of p0's camera on the same X; [24]: p0's root and camera
    __shared__ float s_jt[63], s_jc[21], s_ut[42], s_uc[21];      // the joint and keypoint targets and their confidences: the serial loops read them here
    __shared__ int s_ok[24];
    __shared__ int s_flag, s_root_new;

    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const size_t b = blockIdx.x;
    const float* s_pose = s_p;
    const float* s_beta = s_p + 51;

    // ================================================================ the row and the pass-through test (status bit 1, dir_mano_fit's definition)
    int bad_p = 0;
    if (tid < 64) {
        const float x = a.p0[b * 64 + tid];
        s_p[tid] = x;
        bad_p = !finite(x);
    }
    const int bad_t = fit::targets_nonfinite(a, b, tid);
    if (tid < 63) s_jt[tid] = a.joints_t ? a.joints_t[b * 63 + tid] : 0.f;                    // copies: an entry selected out may hold NaN
    if (tid >= 64 && tid < 85) s_jc[tid - 64] = a.joints_conf ? a.joints_conf[b * 21 + tid - 64] : 1.f;
    if (tid >= 128 && tid < 170) s_ut[tid - 128] = a.uv_t ? a.uv_t[b * 42 + tid - 128] : 0.f;
    if (tid >= 192 && tid < 213) s_uc[tid - 192] = a.uv_conf ? a.uv_conf[b * 21 + tid - 192] : 1.f;
    const bool p0_bad = __syncthreads_or(bad_p) != 0;
    const bool in_bad = __syncthreads_or(bad_t) != 0 || p0_bad;

    // ================================================================ forward at p0 (mano_device.h, layers 2 and 4)
    if (tid < 45) s_full[tid] = pca_axis_angle(T, s_pose + 6, tid);
    shape_blend(T, s_beta, s_v, tid);
    if (tid == 64) { int reflect; robust6d(s_pose, L.root, reflect); s_flag = reflect; }
    __syncthreads();
    forward_schedule(L, T, side, center, root_palm, s_full, s_beta, s_v, s_vert, tid);
    if (tid >= 64 && tid < 67) s_pi[tid - 64] = center >= 0 ? 0.f : L.J[tid - 64];       // step 1: the pivot
    __syncthreads();

    const bool pass = in_bad || s_flag != 0;          // no target enters the arithmetic of a row that passes through
    const bool have3d = a.verts_t || a.joints_t;
    const bool step2 = !pass && have3d && args.root;
    const bool step3 = !pass && !have3d && a.uv_t && args.root && args.cam && args.search;
    const bool step4 = !pass && a.uv_t && args.cam && !step3;
    const bool use_uv = !pass && a.uv_t;
    const float cx = L.c[0], cy = L.c[1], cz = L.c[2], px = s_pi[0], py = s_pi[1], pz = s_pi[2];

    // ================================================================ step 2: the cross-covariance, Horn's rotation, the energies
    if (step2) {
        float red[NRED] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
        if (a.verts_t) {
            for (int v = tid; v < NV; v += BT) {
                const float* t = a.verts_t + (b * NV + v) * 3;
                const float w = args.kv * T.weights[16 * v];
                const float x0 = s_vert[3 * v] - cx, x1 = s_vert[3 * v + 1] - cy, x2 = s_vert[3 * v + 2] - cz;
                const float y0 = t[0], y1 = t[1], y2 = t[2];
                const float u0 = w * (x0 - px), u1 = w * (x1 - py), u2 = w * (x2 - pz), g0 = y0 - px, g1 = y1 - py, g2 = y2 - pz;
                red[0] += u0 * g0; red[1] += u0 * g1; red[2] += u0 * g2;
                red[3] += u1 * g0; red[4] += u1 * g1; red[5] += u1 * g2;
                red[6] += u2 * g0; red[7] += u2 * g1; red[8] += u2 * g2;
                const float d0 = x0 - y0, d1 = x1 - y1, d2 = x2 - y2;
                red[9] += w * (d0 * d0 + d1 * d1 + d2 * d2);
                red[10] += w;
            }
        }
#pragma unroll
        for (int e = 0; e < NRED; ++e) { const float s = dir::wave_sum_dpp(red[e]); if (lane == 0) s_red[wave][e] = s; }
    }
    __syncthreads();
    if (step2 && tid == 0) {
        float acc[NRED] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
        if (a.joints_t) {
            for (int j = 0; j < 21; ++j) {
                if (!rigid_joint(j, root_palm)) continue;
                const float c = s_jc[j];
                if (!(c > 0.f)) continue;                        // selected out, never multiplied by 0: the target may hold NaN
                const float* t = s_jt + 3 * j;
                const float w = args.kj * c;
                const float x0 = L.jtr[3 * j] - cx, x1 = L.jtr[3 * j + 1] - cy, x2 = L.jtr[3 * j + 2] - cz;
                const float y0 = t[0], y1 = t[1], y2 = t[2];
                const float u0 = w * (x0 - px), u1 = w * (x1 - py), u2 = w * (x2 - pz), g0 = y0 - px, g1 = y1 - py, g2 = y2 - pz;
                acc[0] += u0 * g0; acc[1] += u0 * g1; acc[2] += u0 * g2;
                acc[3] += u1 * g0; acc[4] += u1 * g1; acc[5] += u1 * g2;
                acc[6] += u2 * g0; acc[7] += u2 * g1; acc[8] += u2 * g2;
                const float d0 = x0 - y0, d1 = x1 - y1, d2 = x2 - y2;
                acc[9] += w * (d0 * d0 + d1 * d1 + d2 * d2);
                acc[10] += w;
            }
        }
        float S[9], Q[9];
#pragma unroll
        for (int e = 0; e < NRED; ++e) {
            const float tot = acc[e] + (((s_red[0][e] + s_red[1][e]) + s_red[2][e]) + s_red[3][e]);
            s_sum[e] = tot;
            if (e < 9) S[e] = tot;
        }
        dir::horn_rotation(S, Q);
#pragma unroll
        for (int e = 0; e < 9; ++e) s_Q[e] = Q[e];
    }
    __syncthreads();
    if (step2) {
        float Q[9];
#pragma unroll
        for (int e = 0; e < 9; ++e) Q[e] = s_Q[e];
        float e1 = 0.f;
        if (a.verts_t) {
            for (int v = tid; v < NV; v += BT) {
                const float* t = a.verts_t + (b * NV + v) * 3;
                const float w = args.kv * T.weights[16 * v];
                const float x0 = (s_vert[3 * v] - cx) - px, x1 = (s_vert[3 * v + 1] - cy) - py, x2 = (s_vert[3 * v + 2] - cz) - pz;
                const float d0 = (Q[0] * x0 + Q[1] * x1 + Q[2] * x2 + px) - t[0];
                const float d1 = (Q[3] * x0 + Q[4] * x1 + Q[5] * x2 + py) - t[1];
                const float d2 = (Q[6] * x0 + Q[7] * x1 + Q[8] * x2 + pz) - t[2];
                e1 += w * (d0 * d0 + d1 * d1 + d2 * d2);
            }
        }
        e1 = dir::wave_sum_dpp(e1);
        if (lane == 0) s_e1[wave] = e1;
    }
    __syncthreads();
    if (tid == 0) {
        int root_new = 0;
        if (step2) {
            float e1 = 0.f;
            if (a.joints_t) {
                for (int j = 0; j < 21; ++j) {
                    if (!rigid_joint(j, root_palm)) continue;
                    const float c = s_jc[j];
                    if (!(c > 0.f)) continue;
                    const float* t = s_jt + 3 * j;
                    const float w = args.kj * c;
                    const float x0 = (L.jtr[3 * j] - cx) - px, x1 = (L.jtr[3 * j + 1] - cy) - py, x2 = (L.jtr[3 * j + 2] - cz) - pz;
                    const float d0 = (s_Q[0] * x0 + s_Q[1] * x1 + s_Q[2] * x2 + px) - t[0];
                    const float d1 = (s_Q[3] * x0 + s_Q[4] * x1 + s_Q[5] * x2 + py) - t[1];
                    const float d2 = (s_Q[6] * x0 + s_Q[7] * x1 + s_Q[8] * x2 + pz) - t[2];
                    e1 += w * (d0 * d0 + d1 * d1 + d2 * d2);
                }
            }
            e1 = e1 + (((s_e1[0] + s_e1[1]) + s_e1[2]) + s_e1[3]);
            bool any = false;
#pragma unroll
            for (int e = 0; e < 9; ++e) any |= s_sum[e] != 0.f;
            root_new = s_sum[10] > 0.f && any && e1 <= s_sum[9];
            s_e1[0] = root_new ? e1 : s_sum[9];           // info[1]
        }
        s_root_new = root_new;
    }
    __syncthreads();
    const bool root2 = s_root_new != 0;

    // ================================================================ the joints under the root of step 2, relative to the centre
    if (tid < 21) {
        const float x0 = L.jtr[3 * tid] - cx, x1 = L.jtr[3 * tid + 1] - cy, x2 = L.jtr[3 * tid + 2] - cz;
        const float r0 = x0 - px, r1 = x1 - py, r2 = x2 - pz;
        s_Y[3 * tid + 0] = root2 ? s_Q[0] * r0 + s_Q[1] * r1 + s_Q[2] * r2 + px : x0;
        s_Y[3 * tid + 1] = root2 ? s_Q[3] * r0 + s_Q[4] * r1 + s_Q[5] * r2 + py : x1;
        s_Y[3 * tid + 2] = root2 ? s_Q[6] * r0 + s_Q[7] * r1 + s_Q[8] * r2 + pz : x2;
    }
    __syncthreads();

    // ================================================================ steps 3 and 4: one camera per candidate (step 4: candidate 0 alone, on s_Y itself)
    if (use_uv && tid < 25) {
        const float sc0 = s_p[61], tx0 = s_p[62], ty0 = s_p[63];
        int perm[3] = {0, 1, 2};
        float sg[3] = {1.f, 1.f, 1.f};
        const bool permuted = step3 && tid < 24;
        if (permuted) cube_rotation(tid, perm, sg);
        const float pv[3] = {px, py, pz};
        // X_j: P_k (J - pi) + pi in the search, the joints themselves otherwise
        auto xy = [&](int j, float& x, float& y) {
            if (permuted) {
                const float q0 = s_Y[3 * j + 0] - px, q1 = s_Y[3 * j + 1] - py, q2 = s_Y[3 * j + 2] - pz;
                const float a0 = perm[0] == 0 ? q0 : perm[0] == 1 ? q1 : q2, a1 = perm[1] == 0 ? q0 : perm[1] == 1 ? q1 : q2;
                x = sg[0] * a0 + pv[0]; y = sg[1] * a1 + pv[1];
            } else if (tid == 24) { x = L.jtr[3 * j] - cx; y = L.jtr[3 * j + 1] - cy; }      // p0's own root
            else { x = s_Y[3 * j]; y = s_Y[3 * j + 1]; }
        };
        float D = 0.f, mx = 0.f, my = 0.f, mu = 0.f, mv = 0.f;
        for (int j = 0; j < 21; ++j) {
            const float d = s_uc[j];
            if (!(d > 0.f)) continue;
            float x, y;
            xy(j, x, y);
            const float* t = s_ut + 2 * j;
            D += d; mx += d * x; my += d * y; mu += d * t[0]; mv += d * t[1];
        }
        mx /= D; my /= D; mu /= D; mv /= D;
        float num = 0.f, den = 0.f;
        for (int j = 0; j < 21; ++j) {
            const float d = s_uc[j];
            if (!(d > 0.f)) continue;
            float x, y;
            xy(j, x, y);
            const float* t = s_ut + 2 * j;
            const float dx = x - mx, dy = y - my;
            num += d * (dx * (t[0] - mu) + dy * (t[1] - mv));
            den += d * (dx * dx + dy * dy);
        }
        const float s = num / den, tx = mu - s * mx, ty = mv - s * my;
        float e = 0.f, e_p0 = 0.f;
        for (int j = 0; j < 21; ++j) {
            const float d = s_uc[j];
            if (!(d > 0.f)) continue;
            float x, y;
            xy(j, x, y);
            const float* t = s_ut + 2 * j;
            const float r0 = (s * x + tx) - t[0], r1 = (s * y + ty) - t[1], q0 = (sc0 * x + tx0) - t[0], q1 = (sc0 * y + ty0) - t[1];
            e += d * (r0 * r0 + r1 * r1);
            e_p0 += d * (q0 * q0 + q1 * q1);
        }
        s_cand[tid][0] = e; s_cand[tid][1] = s; s_cand[tid][2] = tx; s_cand[tid][3] = ty; s_cand[tid][4] = e_p0;
        if (tid < 24) s_ok[tid] = den > 0.f && finite(s) && s > 0.f && finite(e);
    }
    __syncthreads();

    // ================================================================ the decision and the outputs
    if (tid == 0) {
        int status = p0_bad ? 2 : (in_bad ? 2 : 0) | s_flag;
        int choice = -1, cam_new = 0, root_new = root2 ? 1 : 0;
        float R1[9], cam[3] = {s_p[61], s_p[62], s_p[63]};
        float info[4] = {0.f, 0.f, 0.f, 0.f};
        if (step2) {
            info[0] = s_sum[9]; info[1] = s_e1[0];
            if (!root2) status |= 8;
            else {
#pragma unroll
                for (int r = 0; r < 3; ++r)
#pragma unroll
                    for (int c = 0; c < 3; ++c) R1[3 * r + c] = s_Q[3 * r] * L.root[c] + s_Q[3 * r + 1] * L.root[3 + c] + s_Q[3 * r + 2] * L.root[6 + c];
            }
        }
        if (use_uv) { info[2] = s_cand[24][4]; info[3] = s_cand[0][4]; }      // after: p0's camera on the joints under the new root, unless a camera is written
        if (step3) {
            int best = -1;
            float eb = 0.f;
            for (int k = 0; k < 24; ++k)
                if (s_ok[k] && (best < 0 || s_cand[k][0] < eb)) { best = k; eb = s_cand[k][0]; }
            if (best >= 0 && eb <= s_cand[24][4]) {
                int perm[3];
                float sg[3];
                cube_rotation(best, perm, sg);
#pragma unroll
                for (int r = 0; r < 3; ++r)
#pragma unroll
                    for (int c = 0; c < 3; ++c) R1[3 * r + c] = sg[r] * L.root[3 * perm[r] + c];
                root_new = 1; cam_new = 1; choice = best;
                cam[0] = s_cand[best][1]; cam[1] = s_cand[best][2]; cam[2] = s_cand[best][3];
                info[3] = eb;
            } else {
                status |= 8 | 16;
                info[3] = s_cand[24][4];
            }
        }
        if (step4) {
            if (s_ok[0] && s_cand[0][0] <= s_cand[0][4]) {
                cam_new = 1;
                cam[0] = s_cand[0][1]; cam[1] = s_cand[0][2]; cam[2] = s_cand[0][3];
                info[3] = s_cand[0][0];
            } else status |= 16;
        }
        if (root_new) {
            s_p[0] = R1[0]; s_p[1] = R1[3]; s_p[2] = R1[6];
            s_p[3] = R1[1]; s_p[4] = R1[4]; s_p[5] = R1[7];
        }
        if (cam_new) { s_p[61] = cam[0]; s_p[62] = cam[1]; s_p[63] = cam[2]; }
        if (a.status) a.status[b] = status;
        if (a.choice) a.choice[b] = choice;
        if (a.info) {
#pragma unroll
            for (int e = 0; e < 4; ++e) a.info[b * 4 + e] = info[e];
        }
    }
    __syncthreads();
    if (tid < 64) a.p_out[b * 64 + tid] = s_p[tid];
}

}  // namespace

extern "C" int dir_mano_fit_start(const dir_mano_tables* tables_host, const dir_mano_fit_start_hand* hands_host,
                                  const dir_mano_fit_start_opts* opts_host, int hands, int B, void* stream) {
    using namespace dir;
    if (B == 0) return DIR_OK;
    DIR_REQUIRE(B > 0 && (hands == 1 || hands == 2) && tables_host && hands_host && opts_host, "dir_mano_fit_start: bad arguments");
    const dir_mano_fit_start_opts& o = *opts_host;
    for (float w : {o.w_verts, o.w_joints}) DIR_REQUIRE(w >= 0.f && w <= 3.4e38f, "dir_mano_fit_start: weights must be finite and >= 0");
    StartArgs a;
    for (int h = 0; h < hands; ++h) {
        const dir_mano_tables& t = tables_host[h];
        if (int rc = mano::check_mano_tables(t, "dir_mano_fit_start")) return rc;
        const dir_mano_fit_start_hand& f = hands_host[h];
        DIR_REQUIRE(f.p0 && f.p_out, "dir_mano_fit_start: null pointer (p0 / p_out)");
        DIR_REQUIRE((!f.joints_conf || f.joints_t) && (!f.uv_conf || f.uv_t), "dir_mano_fit_start: confidences without their target");
        a.t[h] = t;
        a.h[h] = f;
    }
    if (hands == 1) { a.t[1] = a.t[0]; a.h[1] = a.h[0]; }
    a.kv = (float)((double)o.w_verts / 778.0); a.kj = (float)((double)o.w_joints / 21.0);
    a.root = o.root != 0; a.cam = o.cam != 0; a.search = o.search != 0;
    DIR_LAUNCH(mano_fit_start_kernel, dim3(B, hands), dim3(BT), 0, (hipStream_t)stream, a);
    return check_launch("dir_mano_fit_start");
}
