/*
 * libdir_hip.so -- C ABI of the MI355X (gfx950) implementation of DIR's iterative-refinement hot path.
 *
 * The reference (PengfeiRen96/DIR) has no FFI: its boundary is Python nn.Module classes.
 * This header is therefore build-defined.  Each entry point names the reference function it replaces
 * (file:line relative to the reference tree); the Python modules under dir_amd/ that mirror the
 * reference classes are thin ctypes callers of exactly these symbols (binding shown in INTEGRATION.md).
 *
 * Conventions
 *   - every pointer is a DEVICE pointer owned by the caller unless the name ends in _host;
 *   - `stream` is a hipStream_t passed as void* (NULL = default stream); all work is enqueued
 *     asynchronously on it, nothing synchronises, nothing is allocated (graph-capture safe);
 *   - tensors are dense row-major float32 unless stated; feature maps are NHWC ("channels last");
 *   - return value: 0 = OK, <0 = DIR_E_* ; dir_last_error() gives a message for the calling thread;
 *   - no entry point throws or aborts.
 */
#ifndef DIR_HIP_H
#define DIR_HIP_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define DIR_OK 0
#define DIR_E_INVALID (-1)  /* bad argument (null pointer, unsupported shape) */
#define DIR_E_LAUNCH (-2)   /* hipLaunchKernel / HIP runtime error          */
#define DIR_E_NODEVICE (-3) /* no gfx950 device visible                     */

#define DIR_ABI_VERSION 57

int dir_abi_version(void);
const char* dir_last_error(void);
/* number of visible HIP devices, and the gcnArchName of device 0 copied into buf (host). */
int dir_device_info(char* arch_host, int arch_len, int* num_cu_host);
/* Measurement aid (bench.py's live roofline): the library notes the name of every kernel it launches for the calling thread.
 * dir_launch_log_reset() clears the note pad; dir_launch_log_get() copies the names launched since then into buf_host as a
 * comma-separated list (kernel names as rocprofv3 reports them, template arguments dropped) and returns how many there were. */
void dir_launch_log_reset(void);
int dir_launch_log_get(char* buf_host, int len);
/* as if `times` launches of kernel `name` had been noted: the counter dir_launch_log_get() returns SATURATES at INT_MAX (a serving process
 * never resets it), only the first 32 names since the last reset are kept.  Used by the CPU tests; launches nothing. */
void dir_launch_log_note(const char* name, long long times);
/* Measurement aid (bench.py `roofline.measured_ceilings`; nothing in the reference, nothing in the product path): ONE launch of a ceiling probe
 * on `stream`.  mode 0: bf16 MFMA loop on pseudo-random operands held in registers (16 x v_mfma_f32_32x32x16_bf16 per wave and iteration, 8 waves
 * per CU, every CU), `iters` iterations; mode 1: 16-byte loads streaming `bytes` of `buf` (larger than the Infinity Cache to price HBM).  `buf`: any
 * device buffer >= 64 bytes (mode 0 only needs a sink); mode 2 (round 5): the first half of `buf` copied to the second half (a streaming kernel reads AND
 * writes: the read-only loop under-reports the HBM ceiling); mode 3: mode 0 on v_mfma_f32_32x32x16_f16 with pseudo-random f16 operands.  Returns the
 * FLOPs (modes 0, 3) / bytes read (mode 1) / bytes read + written (mode 2) of the launch, negative = error code.  Round 6: mode 2's `iters` selects the
 * copy shape (0 = the shipped one); mode 4: every workgroup (2 per CU) streams the SAME first `bytes` of buf `iters` times -- the aggregate L2 -> CU
 * rate at which a small-map convolution's weights reach all CUs; mode 5: ds_read_b128 from a 64 KB LDS tile, 8 waves per CU, `iters` passes of 16
 * reads per lane.  Both return bytes delivered. */
long long dir_probe_launch(int mode, void* buf, long long bytes, int iters, void* stream);

/* ------------------------------------------------------------------------------------------------
 * a8 + a9: MANO forward + weak-perspective projection
 * replaces manopth/manopth/manolayer.py:110-270 (ManoLayer.forward in the configuration of
 * models/dir.py:221-224: 6D root rotation "robust" variant rot6d.py:26-51, 45 PCA pose components,
 * Rodrigues via quaternion rodrigues_layer.py:43-54, LBS, fingertips, joint reorder, root centring)
 * and utils/utils.py:47-63 (projection_batch_xy).
 *
 * Tables (float32, device).  Layouts are k-major so the blend-shape contractions read coalesced:
 *   shapedirs_t [10][2336]   = th_shapedirs[778,3,10]  transposed, rows zero-padded 2334 -> 2336 (index v*3+c)
 *   posedirs_t  [135][2336]  = th_posedirs[778,3,135]  transposed, rows zero-padded (16-byte aligned rows)
 *   v_template  [2334]
 *   j_template  [16][3]      = th_J_regressor @ th_v_template            (folded once, in fp64)
 *   j_shapedirs [16][3][10]  = th_J_regressor @ th_shapedirs              (J is linear in beta)
 *   weights     [778][16]
 *   hands_mean  [45]
 *   comps       [45][45]      th_selected_comps (row k = PCA component k)
 */
typedef struct dir_mano_tables {
    const float* shapedirs_t;
    const float* posedirs_t;
    const float* v_template;
    const float* j_template;
    const float* j_shapedirs;
    const float* weights;
    const float* hands_mean;
    const float* comps;
    int32_t side;       /* 0 = right (tip vertex 444), 1 = left (tip vertex 445): manolayer.py:249-252 */
    int32_t center_idx; /* joint (after reorder) subtracted from verts and joints; -1 = none          */
    int32_t root_palm;  /* !=0: joint 0 = (v95 + v22)/2 instead of the wrist (manolayer.py:253-255)   */
} dir_mano_tables;

/* pose  : B rows of 51 floats (6D root | 45 PCA coeffs), row stride pose_stride floats
 * betas : B rows of 10 floats, row stride betas_stride
 * cam   : optional (NULL ok) B rows of 3 floats (scale, tx, ty), row stride cam_stride
 * verts [B,778,3], joints [B,21,3] metres.  joint_uv [B,21,2] / mesh_uv [B,778,2] optional,
 * written only when cam != NULL.  flags_out (optional, int32[B]): bit0 set when the 6D root matrix
 * has det < 0 (the reference raises AssertionError there, rot6d.py:50; the wrapper re-raises it). */
int dir_mano_forward(const dir_mano_tables* tables_host, const float* pose, int pose_stride,
                     const float* betas, int betas_stride, const float* cam, int cam_stride,
                     float* verts, float* joints, float* joint_uv, float* mesh_uv, int32_t* flags_out,
                     int B, void* stream);

/* Both hands of one stage in ONE launch (grid = B x 2).  tables_lr[2] = {left, right}; the *_lr arguments are HOST
 * arrays of two device pointers.  cam_lr / joint_uv_lr / mesh_uv_lr / flags_lr may be NULL (mesh_uv_lr: pd_mesh_uv_* [B,778,2], which only
 * the training loss reads, models/dir.py:278-280,574-575); flags_lr[h] = int32[B] as flags_out above
 * (the reflection check of rot6d.py:50 that DIR.forward turns into the reference's AssertionError). */
int dir_mano_forward_pair(const dir_mano_tables* tables_lr_host, const float* const* pose_lr_host, int pose_stride,
                          const float* const* betas_lr_host, int betas_stride, const float* const* cam_lr_host,
                          int cam_stride, float* const* verts_lr_host, float* const* joints_lr_host,
                          float* const* joint_uv_lr_host, float* const* mesh_uv_lr_host, int32_t* const* flags_lr_host, int B,
                          void* stream);

/* SURVEY 8f rank 2, backward pass, first link behind the loss gradients: the gradient of
 *   <g_verts, verts> + <g_joints, joints> + <g_joint_uv, joint_uv> + <g_mesh_uv, mesh_uv>
 * w.r.t. pose [B,51], betas [B,10] and cam [B,3] of dir_mano_forward -- what torch autograd computes through
 * manopth/manopth/manolayer.py:110-270 and utils/utils.py:47-63 in the reference's training step (train.py:66-70).
 * The *_lr arguments are HOST arrays of `hands` (1 or 2) device pointers; any g_* input may be NULL (or hold NULL) = no
 * contribution.  Inputs as for the forward (the forward is recomputed, nothing has to be saved).  Deterministic (no atomics). */
int dir_mano_backward_pair(const dir_mano_tables* tables_lr_host, const float* const* pose_lr_host, int pose_stride,
                           const float* const* betas_lr_host, int betas_stride, const float* const* cam_lr_host, int cam_stride,
                           const float* const* g_verts_lr_host, const float* const* g_joints_lr_host,
                           const float* const* g_joint_uv_lr_host, const float* const* g_mesh_uv_lr_host,
                           float* const* g_pose_lr_host, int g_pose_stride, float* const* g_betas_lr_host, int g_betas_stride,
                           float* const* g_cam_lr_host, int g_cam_stride, int hands, int B, void* stream);

/* ------------------------------------------------------------------------------------------------
 * MANO fitting (ABI 52; nothing in the reference): dir_mano_forward run the other way.  Per (sample, hand) the 64-vector p = pose 51 (6D root |
 * 45 PCA) | betas 10 | cam 3 -- the layout of pd_mano_para_* and of dir_mano_backward_pair -- is moved by `iters` Adam steps down
 *
 *   E(p) = w_verts  / 778 * sum_v       |V_v - V*_v|^2
 *        + w_joints / 21  * sum_j c_j   |J_j - J*_j|^2
 *        + w_uv     / 21  * sum_j d_j   |U_j - U*_j|^2
 *        + w_pca * |p[6:51]|^2 + w_beta * |p[51:61]|^2 + w_init * |p - a|^2
 *
 * V(p) [778,3], J(p) [21,3], U(p) [21,2] are dir_mano_forward's verts, joints and joint_uv for the given tables (center_idx, side and root_palm as
 * the caller set them: 3-D targets are relative to the same joint; there is no translation variable).  a = `anchor`, or p0 where it is NULL.
 * A NULL target drops its term; NULL confidences are all 1.  A target whose confidence is not > 0 is selected out, never multiplied by 0: it
 * may hold NaN (a missing keypoint).
 *
 * One iteration, in this order, fp32 throughout (one launch runs all of them; one 256-thread workgroup per (sample, hand) keeps the hand in LDS):
 *   1. the forward at p: the device functions dir_mano_forward runs (csrc/mano_device.h holds the layer once, for every kernel that runs it);
 *   2. the cotangents gV = k_v (V - V*), gJ = (k_j c_j) (J_j - J*_j), gU = (k_uv d_j) (U_j - U*_j), 0 where selected out, with
 *      k_v = 2 w_verts / 778, k_j = 2 w_joints / 21, k_uv = 2 w_uv / 21 formed in double on the host and rounded to float once;
 *   3. g = dir_mano_backward_pair's gradient for these cotangents (the same device functions; 64-lane sums on DPP row operations, fixed order; with
 *      root_palm, which that entry point rejects, joint 0 = (v95 + v22) / 2 hands half its gradient to each of the two vertices);
 *   4. g[6:51] += (2 w_pca) p, then g[51:61] += (2 w_beta) p, then g += (2 w_init) (p - a), each product and sum rounded (no FMA contraction);
 *   5. Adam, step t = t0 + 1 .. t0 + iters, per component of group G (root 0:6, pca 6:51, betas 51:61, cam 61:64), no FMA contraction:
 *        m = b1 * m + (1 - b1) * g            v = b2 * v + (1 - b2) * (g * g)
 *        P1 = P1 * b1, P2 = P2 * b2           (running fp32 products b1^t, b2^t, 1 at t = 0: the bias corrections are 1 - P1 and 1 - P2)
 *        p = p - (lr_G * (m / (1 - P1))) / (sqrt(v / (1 - P2)) + eps)
 *      a group with lr_G == 0 keeps its components bit for bit (m and v still move).
 * The iteration count is fixed: no early stop, no host read, no data-dependent bound (one exception: status bit 2 below ends the row's loop).
 *
 * status (int32 per row, optional):
 *   bit 0  the final iterate's 6D root is a reflection (flags_out's meaning in dir_mano_forward);
 *   bit 1  p0 or `anchor` is non-finite, or a target in use (term present and confidence > 0; the confidence included) is non-finite: the row
 *          passes through -- p_out = p0 bit for bit, its state is untouched, verts / joints / joint_uv are the forward at p0 and mse is 0 (all of
 *          them 0 where p0 itself is non-finite);
 *   bit 2  a step gave a non-finite component of p, m or v: that step is not taken, the iterate before it (the last finite one) is returned with
 *          its state, and the row's loop ends there.
 *
 * mse [B,6] (optional): the unweighted mean squared residuals (verts, joints, joint_uv) at p0, then at the returned p:
 *   sum_v |V_v - V*_v|^2 / 778, sum_{c_j > 0} |J_j - J*_j|^2 / #{c_j > 0}, the same for U; 0 where the term is absent or nothing is selected.
 * state [B, DIR_MANO_FIT_STATE] (optional, in and out): m [64] | v [64] | P1 | P2 | t (the int32's bits) | 0.  All zeros is the fresh state.
 *   With it (and `anchor` held fixed), iters = a followed by iters = b equals iters = a + b bit for bit.
 * p_out may alias p0.  verts [B,778,3], joints [B,21,3], joint_uv [B,21,2] (optional): V, J, U at the returned p.
 * Every reduction runs in a fixed order, no atomics, no workspace: a row gives the same bits in any slot of any batch and in either hand slot. */
#define DIR_MANO_FIT_STATE 132
typedef struct dir_mano_fit_hand {
    const float* p0;          /* [B,64] start                                             */
    const float* anchor;      /* [B,64] centre of the w_init term, or NULL = p0           */
    float* p_out;             /* [B,64] fitted parameters (may alias p0)                   */
    const float* verts_t;     /* V* [B,778,3] or NULL                                      */
    const float* joints_t;    /* J* [B,21,3] or NULL                                       */
    const float* joints_conf; /* c  [B,21] or NULL (= 1)                                   */
    const float* uv_t;        /* U* [B,21,2] or NULL                                       */
    const float* uv_conf;     /* d  [B,21] or NULL (= 1)                                   */
    float* verts;             /* optional outputs at the returned p                        */
    float* joints;
    float* joint_uv;
    float* mse;               /* [B,6] or NULL                                             */
    int32_t* status;          /* [B] or NULL                                               */
    float* state;             /* [B,DIR_MANO_FIT_STATE] in and out, or NULL                */
} dir_mano_fit_hand;
typedef struct dir_mano_fit_opts {
    float w_verts, w_joints, w_uv, w_pca, w_beta, w_init;
    float lr[4];              /* root, pca, betas, cam                                      */
    float b1, b2, eps;        /* 0.9, 0.999, 1e-8 are the defaults of the Python callers    */
    int32_t iters;
} dir_mano_fit_opts;
/* tables_host / hands_host: HOST arrays of `hands` (1 or 2) entries; grid = B x hands.  Enqueued on `stream`, graph-capture safe. */
int dir_mano_fit(const dir_mano_tables* tables_host, const dir_mano_fit_hand* hands_host, const dir_mano_fit_opts* opts_host,
                 int hands, int B, void* stream);

/* ------------------------------------------------------------------------------------------------
 * MANO fitting: closed-form start (ABI 54; csrc/mano_fit_start.hip; nothing in the reference).  Adam takes lr-sized steps, so a fit that starts
 * at the identity root spends its iterations turning the wrist and never reaches a far rotation.  dir_mano_fit_start moves p0's ROOT (6 floats)
 * and CAMERA (3 floats) to where a closed form puts them and copies the other 55 floats; dir_mano_fit then starts from p_out.  One launch, one
 * 256-thread workgroup per (sample, hand), ONE forward at p0 (the forward phases of csrc/mano_device.h), everything after it closed form.  fp32
 * throughout, every sum in a fixed order, no atomics, no workspace, no host read, graph-capture safe; a row gives the same bits in any slot of
 * any batch and in either hand slot.  tests/helpers/mano_start_ref.py restates the rule in torch.
 *
 * Per row.  R0 = the robust-6D rotation of p0[0:6]; V [778,3], J [21,3] = dir_mano_forward's verts and joints at p0 (centred as the tables say).
 *   0. Pass-through.  p0 non-finite, or a target in use non-finite (dir_mano_fit's status bit 1, the same definition: a term is in use when its
 *      pointer is given, an entry when its confidence is > 0): p_out = p0 bit for bit, status bit 1, choice -1, info 0.  R0 a reflection: the same
 *      with status bit 0.
 *   1. Pivot.  pi = 0 when center_idx >= 0, else the rest-pose chain joint 0 at p0's betas (j_template + j_shapedirs beta, row 0).  Multiplying
 *      the root from the left by a rotation Q maps every output X to Q (X - pi) + pi (to ~1e-9 m: a float32 skinning row does not sum to 1).
 *   2. Root from 3-D targets -- when verts_t or joints_t is given and opts.root != 0.  Over the points that are rigid under the root:
 *        joints    RS = {0, 1, 5, 9, 13, 17} (wrist, thumb base, the four MCPs; pd_joint_xyz_* order), without joint 0 when root_palm; weight
 *                  w_j = k_j c_j for c_j > 0 (c_j <= 0: selected out, never multiplied, may hold NaN), k_j = w_joints / 21;
 *        vertices  all 778, weight w_v = k_v * weights[v][0] (the root's skinning weight), k_v = w_verts / 778;
 *      k_j, k_v formed in double on the host and rounded once.  With x the model point and y its target:
 *        S[a][b] = sum w (x - pi)_a (y - pi)_b      e0 = sum w |x - y|^2      W = sum w
 *      each as (the joints of RS in index order, from 0) + (the vertices: lane t adds v = t, t + 256, ... in order, then the DPP tree of each
 *      64-lane wave, then the four waves in order).  Q = the Horn rotation of S (csrc/horn_rotation.h, the one dir_procrustes_align runs);
 *      e1 = sum w |Q (x - pi) + pi - y|^2 in the same order.  If W is not > 0, or S is all zero, or e1 is not <= e0: the root keeps p0's six
 *      bits and status bit 3 (value 8) is set.  Otherwise R1 = Q R0 and p_out[0:6] = columns 0 and 1 of R1.
 *      (Centring at a finger joint biases this, because the pivot then moves with the pose: accepted, it is a start.)
 *   3. Root from 2-D targets only -- when neither verts_t nor joints_t is given, uv_t is given and opts.root, opts.cam and opts.search are all
 *      != 0 (a candidate is scored under its own camera, so both groups are written or neither).  The candidates are the 24 proper rotations of
 *      the cube: permutations `perm` of (0, 1, 2) in lexicographic order, within each the sign triples sg in the order (+,+,+), (+,+,-), (+,-,+),
 *      ...; row r of P has sg[r] at column perm[r]; the ones with det +1 are kept and numbered k = 0 .. 23 in that order (k = 0 is the identity).
 *      Candidate joints are P_k (J - pi) + pi; each candidate gets the camera of step 4 on them and e_k = its 2-D residual.  A candidate whose
 *      denominator is not > 0, whose s is not finite and > 0 or whose e_k is not finite is dropped (s <= 0 is the mirrored camera).  The
 *      smallest e_k wins, ties to the lowest k.  If nothing survives, or the best e_k is not <= the residual of p0's own root and camera, root and camera keep p0's bits, status
 *      bits 3 and 4 are set and choice = -1.  Otherwise R1 = P_k R0, p_out[0:6] = its columns 0 and 1, the camera is the candidate's, choice = k.
 *   4. Camera -- when uv_t is given and opts.cam != 0 (and step 3 did not run).  X_j = the xy of the joints under the root of step 2 (J itself
 *      where that step did not run or kept p0's root, else Q (J - pi) + pi), over the keypoints with d_j > 0 in index order:
 *        D = sum d    Xm = sum d X / D    Um = sum d U / D    s = sum d (X - Xm).(U - Um) / sum d |X - Xm|^2    t = Um - s Xm
 *      (dir_mano_forward's uv = s xy + t).  Accepted only if the denominator is > 0, s is finite and > 0 and its residual sum d |s X + t - U|^2
 *      is finite and <= the residual of p0's camera on the same X; otherwise p0's three bits stay and status bit 4 (value 16) is set.
 *   5. The 45 PCA coefficients and the 10 betas are copied bit for bit, and so is every group whose switch is off.  p_out may alias p0.
 * status (int32 per row, optional): bit 0 and bit 1 as above (step 0), bit 3 the root was not moved by a step that ran, bit 4 the camera was not.
 * choice (int32 per row, optional): the candidate step 3 wrote, -1 otherwise.
 * info [B,4] (optional): the weighted 3-D energy e0, then e1 (e0 again where the root was kept; 0, 0 where step 2 did not run); then the 2-D
 *   residual sum d |s X + t - U|^2 at p0's root and camera, then at p_out's (0, 0 without uv_t). */
typedef struct dir_mano_fit_start_hand {
    const float* p0;          /* [B,64] start                                             */
    float* p_out;             /* [B,64] (may alias p0)                                     */
    const float* verts_t;     /* V* [B,778,3] or NULL                                      */
    const float* joints_t;    /* J* [B,21,3] or NULL                                       */
    const float* joints_conf; /* c  [B,21] or NULL (= 1)                                   */
    const float* uv_t;        /* U* [B,21,2] or NULL                                       */
    const float* uv_conf;     /* d  [B,21] or NULL (= 1)                                   */
    int32_t* status;          /* [B] or NULL                                               */
    int32_t* choice;          /* [B] or NULL                                               */
    float* info;              /* [B,4] or NULL                                             */
} dir_mano_fit_start_hand;
typedef struct dir_mano_fit_start_opts {
    float w_verts, w_joints;  /* the weights of the two 3-D terms against one another       */
    int32_t root, cam, search;/* switches: != 0 = the step may write its group              */
} dir_mano_fit_start_opts;
/* tables_host / hands_host: HOST arrays of `hands` (1 or 2) entries; grid = B x hands.  Enqueued on `stream`. */
int dir_mano_fit_start(const dir_mano_tables* tables_host, const dir_mano_fit_start_hand* hands_host, const dir_mano_fit_start_opts* opts_host,
                       int hands, int B, void* stream);

/* ------------------------------------------------------------------------------------------------
 * MANO fitting: sequences (ABI 56; csrc/mano_fit_seq.hip; nothing in the reference).  dir_mano_fit fits every row alone.  Keypoint tracks come as
 * sequences of one person: dir_mano_fit_sequence is ONE optimisation over a batch of sequences that keeps one shape per (sequence, hand), a pose
 * and a camera per frame, and couples neighbouring frames in time.  tests/helpers/mano_seq_fit_ref.py restates the rule in torch.
 *
 * A batch is S sequences laid end to end: seq_start [S+1] int32 ON THE DEVICE, ascending, seq_start[0] = 0, seq_start[S] = N; frames
 * seq_start[s] .. seq_start[s+1] - 1 are sequence s (a sequence may have length 1).  The arrays of dir_mano_fit_hand have N rows.
 *
 * Frame classes, decided once from the inputs (bits of `status`):
 *   inert    (bit 1)      p0 or `anchor` non-finite.  The frame passes through as dir_mano_fit's bit-1 rows do (p_out = p0 bit for bit, state untouched,
 *                         outputs the forward at p0, or 0 where p0 is non-finite, mse 0).  It is in no chain: no temporal edge touches it, its two
 *                         neighbours do NOT become neighbours of each other, and it gives nothing to the shared shape.
 *   no data  (bit 3 = 8)  a target in use (dir_mano_fit's definition) is non-finite: every data term of the frame is dropped; it stays in the chain, and
 *                         priors, temporal terms and the shared shape still move it.  A frame whose confidences are all 0 behaves the same way and
 *                         sets no bit: that is how missing frames are filled.
 * An EDGE joins frames t - 1 and t of one sequence when neither is inert.
 *
 * Variables of one (sequence, hand): per frame the 54 floats root 0:6 | PCA 6:51 | cam 61:64, and the betas 51:61 -- one 10-vector b per sequence with
 * share_betas != 0 (start and prior centre: p0's / anchor's betas of the sequence's first frame that is not inert), else 10 per frame as dir_mano_fit.
 *
 *   E = sum_t E_data(p_t)            dir_mano_fit's E with the same dir_mano_fit_opts; with share_betas the terms w_beta |b|^2 and w_init |b - a_b|^2
 *                                    enter once per sequence, not once per frame
 *     + sum over edges (t-1, t):     w_t_root |R(p_t) - R(p_{t-1})|_F^2  +  w_t_pca |p_t[6:51] - p_{t-1}[6:51]|^2  +  w_t_cam |p_t[61:64] - p_{t-1}[61:64]|^2
 *   R = the robust-6D rotation of the six root floats (dir_mano_forward's): a chordal distance, independent of the scale of the unnormalised 6D input.
 *
 * One iteration = one Adam step on E for every frame at once, every gradient taken at iterate k: the iterates live in two copies in the workspace, a
 * frame reads itself and its neighbours from copy k & 1 and writes copy (k + 1) & 1, and a launch boundary separates the iterations (no grid barrier,
 * no flags).  Per frame and iteration, fp32 throughout:
 *   1-3. dir_mano_fit's steps 1-3 (with share_betas the forward runs at the sequence's b), with one addition before the robust-6D chain rule: with
 *        w_t_root > 0 the 3x3 root cotangent G gets, element by element, G = G + k_r (R - R_prev) where the edge to t - 1 exists, then
 *        G = G + k_r (R - R_next) where the edge to t + 1 exists; k_r = 2 w_t_root; R_prev / R_next = robust 6D of the neighbour's six floats;
 *   4.   dir_mano_fit's step 4 (with share_betas the ten betas are left out: step 6), then for i in 6:51 with w_t_pca > 0:
 *        g_i = g_i + k_p (p_i - prev_i) where the edge to t - 1 exists, then g_i = g_i + k_p (p_i - next_i) where the edge to t + 1 exists, k_p = 2 w_t_pca;
 *        the same for i in 61:64 with k_c = 2 w_t_cam.  Each product and sum rounded (no FMA contraction).  A term whose weight is 0 and a missing
 *        edge are SKIPPED, never multiplied by 0: with the three weights 0 and share_betas = 0 every frame gives dir_mano_fit's bits;
 *   5.   dir_mano_fit's step 5 on the frame's components (54 with share_betas: m and v of 51:61 in the frame's state stay as they are).  A step
 *        that gives a non-finite p, m or v is not taken: status bit 2, the frame is FROZEN at that iterate for the rest of the call (its neighbours
 *        still see it; it gives nothing further to the shape).
 *   6.   With share_betas, per (sequence, hand) after all frames' step 5: g_b[k] = the sum over the sequence's frames that are neither inert nor
 *        frozen (the one frozen in this iteration included in "frozen") of the backward's d E_data / d betas[k] taken at b -- a fixed tree that depends
 *        on the sequence's length only: lane l of 256 adds frames l, l + 256, ... (index within the sequence) in order, excluded frames adding 0.f,
 *        each 64-lane wave sums its lanes (the DPP tree of dir_mano_fit) and the four waves are added in order; no atomics.  Then
 *        g_b = g_b + (2 w_beta) b, g_b = g_b + (2 w_init) (b - a_b), and step 5 on b with lr[2] and the sequence's own m, v, P1, P2.  A non-finite step
 *        is not taken and freezes the shape for the rest of the call (seq_status bit 2).  Every frame of iterate k + 1 reads the same ten floats.
 *
 * iters is fixed: no early stop, no host read; the whole call is 2 + iters (1 + (share_betas != 0)) + 1 launches on `stream` and can be captured in a graph.
 *
 * Outputs (dir_mano_fit_hand's, N rows): p_out (with share_betas the sequence's b in every frame's 51:61 that is not inert; may alias p0), verts /
 * joints / joint_uv at the returned p, mse [N,6] as dir_mano_fit (a no-data frame: 0), status [N]: bit 0 reflection, 1 inert, 2 frozen, 3 no data.
 * state [N, DIR_MANO_FIT_STATE] (optional, in and out) as dir_mano_fit; seq_state (optional, in and out, per hand [S, DIR_MANO_FIT_SEQ_STATE]):
 * m [10] | v [10] | P1 | P2 | t (the int32's bits) | 0 of the shared shape, all zeros = fresh.  With both (and the anchor held fixed), iters = a then
 * iters = b from the first call's p_out equals iters = a + b bit for bit.
 * seq_status [hands, S] int32 (optional): bit 1 = the sequence has no frame in a chain, bit 2 = its shared shape was frozen.
 * A sequence gives the same bits alone, in any slot of any ragged batch, and in either hand slot. */
#define DIR_MANO_FIT_SEQ_STATE 24
#define DIR_MANO_FIT_SEQ_LANES 256 /* the width of step 6's tree */
typedef struct dir_mano_fit_seq_opts {
    float w_t_root, w_t_pca, w_t_cam;   /* >= 0; 0 = the term is absent                                                            */
    int32_t share_betas;                /* != 0: one shape per (sequence, hand)                                                     */
    const int32_t* seq_start_host;      /* optional HOST copy of seq_start [S+1]: when given it is checked (0, ascending, N at the end) */
    float* seq_state[2];                /* per hand: [S, DIR_MANO_FIT_SEQ_STATE] in and out, or NULL                               */
} dir_mano_fit_seq_opts;
/* bytes of `work` for N frames in S sequences (0 on bad arguments).  The contents need no initialisation and mean nothing afterwards. */
size_t dir_mano_fit_sequence_workspace_bytes(int N, int S, int hands);
/* tables_host / hands_host: HOST arrays of `hands` (1 or 2) entries.  seq_start, seq_status, work: device.  Nothing is allocated; a workspace smaller
 * than the query, negative or non-finite weights, or a seq_start_host that is not ascending from 0 to N return DIR_E_INVALID before any launch.  A
 * seq_start on the device that breaks the rule cannot fault (every index is clamped to the N frames) but fits unspecified chains. */
int dir_mano_fit_sequence(const dir_mano_tables* tables_host, const dir_mano_fit_hand* hands_host, const dir_mano_fit_opts* opts_host,
                          const dir_mano_fit_seq_opts* seq_opts_host, const int32_t* seq_start, int S, int N, int hands, int32_t* seq_status,
                          void* work, size_t work_bytes, void* stream);

/* ------------------------------------------------------------------------------------------------
 * MANO fitting: two hands together (ABI 57; csrc/mano_fit_pair.hip; nothing in the reference).  dir_mano_fit fits each hand alone and has no
 * variable for where the right hand is relative to the left.  dir_mano_fit_pair fits B PAIRS: per pair the two 64-vectors p_L, p_R of
 * dir_mano_fit (hands_host[0] = left slot, [1] = right slot) and the 3-vector o = the right hand's centre joint minus the left hand's, metres,
 * camera axes (0.15 * pd_offset of the network).  In the common frame the left joints are X^L_j = J^L_j and the right joints X^R_j = J^R_j + o,
 * J = dir_mano_fit's centred output joints (the output's bits; the sum with o rounded once).  tests/helpers/mano_pair_fit_ref.py restates the rule.
 *
 *   E = E_fit(p_L) + E_fit(p_R)                             dir_mano_fit's E, the same dir_mano_fit_opts for both hands
 *     + w_off * c_o * |o - o*|^2                             o* = o_target; dropped when o_target is NULL or c_o is not > 0 (o* may then hold NaN)
 *     + w_off_init * |o - o_a|^2                             o_a = o_anchor, or o0 where it is NULL
 *     + w_col / 400 * sum_{i<20} sum_{j<20} h_ij^2           h_ij = max(0, (r^L_i + r^R_j) - d_ij)
 *
 * Bones: bone k joins joints parent(k) and child(k) = k + 1, parent = {0,1,2,3, 0,5,6,7, 0,9,10,11, 0,13,14,15, 0,17,18,19} (csrc/bone_common.h,
 * the reference's Joint2BoneFeature).  radii[0] = r^L, radii[1] = r^R: [20] floats on the device.  d_ij = the distance between the segments
 * (A, B) = (X^L_parent(i), X^L_child(i)) and (C, D) = (X^R_parent(j), X^R_child(j)), by Ericson's closest points of two segments, fp32, every
 * operation rounded (no FMA contraction), dot products summed x, y, z left to right, clamp(x) = x < 0 ? 0 : x > 1 ? 1 : x:
 *     d1 = B - A, d2 = D - C, r = A - C, a = d1.d1, e = d2.d2, f = d2.r, eps = 1e-12 (m^2: a segment shorter than 1 um is a point)
 *     if a <= eps and e <= eps:   s = 0, t = 0
 *     else if a <= eps:           s = 0, t = clamp(f / e)
 *     else: c = d1.r
 *        if e <= eps:             t = 0, s = clamp(-c / a)
 *        else: b = d1.d2, den = a e - b b
 *             s = den != 0 ? clamp((b f - c e) / den) : 0          (parallel segments: s = 0)
 *             t = (b s + f) / e
 *             if t < 0:           t = 0, s = clamp(-c / a)
 *             else if t > 1:      t = 1, s = clamp((b - c) / a)
 *     c1 = A + s d1, c2 = C + t d2, w = c1 - c2, d = sqrt(w.w), n = w / d
 * A pair with d finite and >= 1e-6 and h > 0 is ACTIVE.  A pair with d not finite contributes nothing; a pair with d < 1e-6 and h > 0 (the segments
 * cross: no direction) contributes h to the report below and no gradient; both set pair_status bit 3.  Every other pair (h = 0) is skipped.
 *
 * One iteration: dir_mano_fit's steps 1-5 for both hands at the same iterate, with these additions, and only while the coupling is on (below):
 *   2a. (between steps 2 and 3, only with w_col > 0) for every active pair, with u = k_col h, k_col = 2 w_col / 400 formed in double on the host and
 *       rounded once -- the envelope gradient, s and t held fixed, every product rounded:
 *         gA = -(u (1 - s)) n     gB = -(u s) n     gC = (u (1 - t)) n     gD = (u t) n     g_pair = gC + gD
 *       per left bone i: GA_i = sum_j gA, GB_i = sum_j gB, go_i = sum_j g_pair over the active j ascending (from 0.f); per right bone j: GC_j, GD_j over
 *       the active i ascending.  Then per hand and joint q: gJ_q = gJ_q + (the sum, from 0.f, over the bones k ascending that have an active pair
 *       of: the parent-end sum where parent(k) = q, the child-end sum where child(k) = q), and the hand's sum of all cotangents (what centre() hands
 *       to the centre joint) S = S + (the sum over the same bones k ascending of parent-end + child-end).  A bone without an active pair and a
 *       joint without such a bone are skipped, never added as zero.  g_o = the sum over i ascending of go_i for the bones i with an active pair.
 *   4a. g_o = g_o + (k_off c_o) (o - o*) where the target is in use, then g_o = g_o + k_oi (o - o_a); k_off = 2 w_off, k_oi = 2 w_off_init.
 *   5a. step 5 on the three components of o with lr_o and o's own m, v, P1, P2, t (a fifth group).  lr_o == 0 keeps o bit for bit.
 *
 * Rows.  The coupling of a pair is ON when neither hand passes through (dir_mano_fit's status bit 1) and o0, o_a, the target in use (c_o included)
 * and the 40 radii are finite.  Otherwise o passes through (offset_out = o0 bit for bit, its state untouched), no term above the two E_fit exists,
 * col is 0, and each hand is fitted exactly as dir_mano_fit fits it.  A hand frozen by a non-finite step (status bit 2) stays where it is as an
 * obstacle while the other hand and o go on.  A non-finite step of o is not taken and freezes o at its last finite value (the collision term stays).
 * pair_status (int32 per pair, optional): bit 0 a hand passes through: coupling off; bit 1 o0 / o_a / o* / c_o / radii non-finite: coupling off;
 *   bit 2 o frozen by a non-finite step; bit 3 a pair without direction (or with a non-finite distance) was met at an evaluated iterate.
 * With w_col = 0, no o_target, w_off_init = 0 and lr_o = 0, and whenever no pair is active, both hands' outputs and states are dir_mano_fit's bits.
 *
 * Outputs on top of each hand's dir_mano_fit outputs: offset_out [B,3] (may alias o0); col [B,4] (optional) = (sum_i (sum_j h_ij^2)) / 400 and max h_ij
 * in metres (i ascending, j ascending inside; max from 0) at the start, then the same two at the returned iterate: with iters = 0 the call is the
 * measure alone, and the measure does not depend on w_col.  o_state [B, DIR_MANO_FIT_PAIR_STATE] (optional, in and out): m [3] | v [3] | P1 | P2 |
 * t (the int32's bits) | 0 0 0; it follows the two hands' DIR_MANO_FIT_STATE blocks (hands_host[h].state), which keep dir_mano_fit's layout, so a
 * hand's state moves between the two entry points.  With all three, iters = a then iters = b equals iters = a + b bit for bit.
 * One launch, one 512-thread workgroup per pair (threads 0-255 the left slot, 256-511 the right, each through dir_mano_fit's phases), fp32, no
 * atomics, no workspace, no allocation, no host read; enqueued on `stream`, graph-capture safe; a pair gives the same bits in any slot of any batch. */
#define DIR_MANO_FIT_PAIR_STATE 12
typedef struct dir_mano_fit_pair_args {
    const float* o0;          /* [B,3] start                                               */
    const float* o_target;    /* o* [B,3] or NULL                                          */
    const float* o_conf;      /* c_o [B] or NULL (= 1)                                     */
    const float* o_anchor;    /* o_a [B,3] or NULL = o0                                    */
    const float* radii[2];    /* r^L, r^R: [20] each                                       */
    float* offset_out;        /* [B,3] (may alias o0)                                      */
    float* col;               /* [B,4] or NULL                                             */
    int32_t* pair_status;     /* [B] or NULL                                               */
    float* o_state;           /* [B,DIR_MANO_FIT_PAIR_STATE] in and out, or NULL           */
} dir_mano_fit_pair_args;
typedef struct dir_mano_fit_pair_opts {
    float w_col, w_off, w_off_init, lr_o;   /* finite and >= 0 */
} dir_mano_fit_pair_opts;
/* tables_host / hands_host: HOST arrays of exactly two entries (left slot, right slot). */
int dir_mano_fit_pair(const dir_mano_tables* tables_host, const dir_mano_fit_hand* hands_host, const dir_mano_fit_opts* opts_host,
                      const dir_mano_fit_pair_args* pair_host, const dir_mano_fit_pair_opts* pair_opts_host, int B, void* stream);

/* Backward of RegressorOffset's three Linears (models/dir.py:339-351).  w_left / w_right [64][1408], w_offset [3][2691]: the
 * nn.Linear weights in their own layout; tok [B,42,64] = the STE head output (tokens 0..20 left); prev_* the previous stage's
 * (detached) mano_para [B,64] / offset [B,3]; g_para_* [B,64], g_offset [B,3]: gradients w.r.t. the Linears' outputs.
 * Outputs (gw_* / gb_* in the parameters' layout, written not accumulated; all six or none) and g_tok [B,42,64] (optional). */
int dir_regress_backward(const float* w_left, const float* w_right, const float* w_offset, const float* tok,
                         const float* prev_para_left, const float* prev_para_right, const float* prev_offset,
                         const float* g_para_left, const float* g_para_right, const float* g_offset,
                         float* gw_left, float* gb_left, float* gw_right, float* gb_right, float* gw_offset, float* gb_offset,
                         float* g_tok, int B, void* stream);

/* ------------------------------------------------------------------------------------------------
 * building blocks of the backward pass over the joint-token path (train.py:66-70 runs torch autograd through
 * transformer/mixSTE.py, SemGCN/p_graph_conv.py and the Conv1d / Linear / LayerNorm / BatchNorm1d modules of models/dir.py:19-130).
 * Exact fp32, deterministic (fixed summation orders, no atomics); composed on the host by dir_amd/train/.
 */
/* C[b] (+)= op(A[b]) op(B[b]) (+ bias[n]):  op(X) = X or X^T; row-major, leading dimensions in elements, `batch` problems
 * `stride_*` elements apart.  trans_a = 0: A is [M][K]; 1: A is [K][M].  trans_b = 0: B is [K][N]; 1: B is [N][K] (nn.Linear weight).
 * accumulate != 0: C += product + bias (a residual branch lands on its trunk in place).  v_mfma_f32_16x16x4_f32: exact fp32
 * products, k ascending.  64 x 64 output tiles, or 32 x 32 when those would be <= 128 workgroups (the joint-token path's products: a wave
 * then owns one 16 x 16 block and the per-step LDS -> MFMA chain is a quarter as long); the k order per element, and so the bits, are the same
 * (DIR_GEMM_SMALL=0 keeps the 64 x 64 tiles). */
typedef struct dir_gemm_desc {
    int32_t M, N, K, lda, ldb, ldc, trans_a, trans_b, accumulate, batch;
    int64_t stride_a, stride_b, stride_c;
} dir_gemm_desc;
int dir_gemm_f32(const dir_gemm_desc* desc_host, const float* A, const float* B, const float* bias, float* C, void* stream);
/* dir_gemm_f32 over an ny x nx grid of GROUPS: group (gy, gx) displaces A, B and C by gy * *_y + gx * *_x elements -- a convolution tap
 * as a pointer shift over a zero-bordered pixel grid (csrc/bonefuse_bwd.hip).  reduce = 0: every (batch entry, group) its own product in
 * ONE launch (batch * ny * nx <= 65535); reduce = 1: C = sum over the groups (in group order, inside one workgroup) of the displaced
 * products; c_y / c_x are ignored.  batch == 1 and one group: the same bits as dir_gemm_f32. */
typedef struct dir_gemm_groups {
    int32_t ny, nx, reduce, reserved;
    int64_t a_y, a_x, b_y, b_x, c_y, c_x;
} dir_gemm_groups;
int dir_gemm_f32_grouped(const dir_gemm_desc* desc_host, const dir_gemm_groups* groups_host, const float* A, const float* B, const float* bias,
                         float* C, void* stream);
/* the same product (batch == 1) with the reduction cut into chunks of 64, one workgroup per (tile, chunk), partial tiles summed in chunk order by a
 * second launch (deterministic): for tall reductions with a small output -- the Linear weight gradients of the token path (K = rows = B * 21 .. 42).
 * Not bit-identical to dir_gemm_f32 (another summation order); workspace of dir_gemm_f32_splitk_workspace_bytes(d) bytes. */
long long dir_gemm_f32_splitk_workspace_bytes(const dir_gemm_desc* desc_host);
int dir_gemm_f32_splitk(const dir_gemm_desc* desc_host, const float* A, const float* B, const float* bias, float* C, float* workspace,
                        long long workspace_bytes, void* stream);
/* out[n] (+)= sum_r x[r][n]: bias gradients.  R > 512: 256-row chunk partials added in chunk order; workspace of
 * dir_colsum_workspace_bytes(R, N) bytes (0 for R <= 512). */
long long dir_colsum_workspace_bytes(int R, int N);
int dir_colsum_f32(const float* x, float* out, int R, int N, int ld, int accumulate, float* workspace, long long workspace_bytes, void* stream);
/* nn.LayerNorm over the last dimension of x [R][C] (C <= 256); mean / rstd [R] are saved for the backward */
int dir_layernorm_forward(const float* x, const float* w, const float* b, float* y, float* mean, float* rstd, int R, int C, float eps, void* stream);
int dir_layernorm_backward(const float* gy, const float* x, const float* w, const float* mean, const float* rstd, float* gx, float* gw,
                           float* gb, int R, int C, int accumulate_x, int accumulate_wb, void* stream);
/* nn.GELU() (exact erf form; transformer/mixSTE.py:12,27) */
int dir_gelu_forward(const float* x, float* y, long long n, void* stream);
int dir_gelu_backward(const float* gy, const float* x, float* gx, long long n, void* stream);
/* Attention.forward without the two Linears (transformer/mixSTE.py:76-97): qkv [B][T][3][H][32] -> out [B][T][H*32] =
 * softmax(q k^T * scale) v per (sample, head); probs [B][H][T][T] is saved for the backward (may be NULL in inference).  T <= 64. */
int dir_attention_forward(const float* qkv, float* probs, float* out, int B, int T, int H, float scale, void* stream);
int dir_attention_backward(const float* qkv, const float* probs, const float* gout, float* gqkv, int B, int T, int H, float scale, void* stream);
/* BatchNorm in TRAINING mode over x [R][C] with row stride ld (channels last: R = samples x positions): batch mean and biased
 * variance, y = (x - mean) * rstd * w + b, running statistics updated with `momentum` and the unbiased variance (torch semantics);
 * save_mean / save_rstd [C] feed the backward, which returns g x (optional), g w, g b (optional).  relu != 0 fuses the nn.ReLU that follows
 * the BatchNorm on the path (models/backbone/resnet.py:122-131, hourglass.py:58-66): the forward writes max(y, 0) and the backward masks gy
 * where the re-computed y is not positive (same expression, same mask as the forward's; it therefore also needs b).  residual (forward,
 * optional, [R][C] with the same row stride): added before the ReLU -- the tail of a ResNet bottleneck, relu(bn3(.) + identity)
 * (models/backbone/resnet.py:136-140); the backward of THAT form masks with the saved output instead (dir_relu_backward) and passes relu = 0.  R <= 512: one
 * thread per channel walks the rows in order, no workspace.  Larger R (BatchNorm2d over feature maps): the column reductions are cut
 * into 256-row chunks whose partials are combined in chunk order (deterministic; the variance as sum_k [M2_k + n_k (mean_k - mean)^2] / R,
 * one pass over HBM); workspace of dir_bn_train_workspace_bytes(R, C). */
long long dir_bn_train_workspace_bytes(int R, int C);
int dir_bn_train_forward(const float* x, const float* w, const float* b, float* y, float* save_mean, float* save_rstd, float* running_mean,
                         float* running_var, int R, int C, int ld, float eps, float momentum, int relu, const float* residual,
                         float* workspace, long long workspace_bytes, void* stream);
int dir_bn_train_backward(const float* gy, const float* x, const float* w, const float* b, const float* save_mean, const float* save_rstd, float* gx,
                          float* gw, float* gb, int R, int C, int ld, int relu, float* workspace, long long workspace_bytes, void* stream);
/* dir_bn_train_backward whose first pass (the two column sums) is replaced by chunk partials a data-gradient convolution's epilogue formed
 * (dir_conv2d_forward_ex): p1 / p2 [chunks][C]; workspace: 2 C floats.  Same combine (chunk order) and apply kernels. */
int dir_bn_train_backward_from_partials(const float* gy, const float* x, const float* w, const float* b, const float* save_mean, const float* save_rstd,
                                        const float* p1, const float* p2, int chunks, float* gx, float* gw, float* gb, int R, int C, int ld, int relu,
                                        float* workspace, long long workspace_bytes, void* stream);
/* round 5 -- BatchNorm2d (training mode) whose output feeds exactly ONE convolution (Bottleneck bn1 / bn2, models/backbone/resnet.py:125-131;
 * every BatchNorm of the pre-activation Residual, models/backbone/hourglass.py:60-67): only the statistics are formed here (the same kernels and bits
 * as dir_bn_train_forward: save_mean, save_rstd, running statistics) plus pre_scale = w rstd and pre_shift = b - mean w rstd [C]; the normalised
 * map is never written -- the consuming convolution applies act(x pre_scale + pre_shift) where it reads x (dir_conv2d_forward's pre_scale /
 * pre_shift + DIR_CONV_PRE_RELU, dir_split_f16_forward's, and dir_conv2d_wgrad_f16x3_pre for its weight gradient).  dir_bn_train_backward is
 * unchanged (it re-computes the ReLU mask from x).  R > 512 rows, C % 4 == 0 (the Python step takes it for C % 32 == 0: whole reduction slabs of the consumer); workspace: dir_bn_train_workspace_bytes(R, C). */
int dir_bn_train_stats(const float* x, const float* w, const float* b, float* save_mean, float* save_rstd, float* pre_scale, float* pre_shift,
                       float* running_mean, float* running_var, int R, int C, int ld, float eps, float momentum, float* workspace,
                       long long workspace_bytes, void* stream);
/* ... from chunk partials the PRODUCING convolution's epilogue formed (dir_conv2d_forward_stats: the map is not read again for its statistics):
 * p1 / p2 [ceil(R / chunk_rows)][C] = per chunk the column sums and the sums of squared deviations from the chunk's own mean; combined in chunk
 * order like dir_bn_train_forward's (deterministic).  pre_scale / pre_shift may both be NULL (a BatchNorm that is applied by dir_bn_train_apply).
 * cap_rows: how many rows of C floats p1 and p2 each have room for; with more than 256 chunks and cap_rows >= chunks + ceil(chunks / 32) the chunks
 * are first pooled in groups of 32 behind the chunk rows (one more launch, both short) -- the buffers are scratch after the call. */
int dir_bn_train_stats_from_partials(float* p1, float* p2, int chunk_rows, int cap_rows, const float* w, const float* b, float* save_mean, float* save_rstd,
                                     float* pre_scale, float* pre_shift, float* running_mean, float* running_var, int R, int C, float eps, float momentum,
                                     void* stream);
/* the normalisation alone from statistics already formed: y = act(BatchNorm(x) + residual), the third launch of dir_bn_train_forward (a Bottleneck's
 * bn3 + identity + ReLU, models/backbone/resnet.py:133-140, whose statistics came out of conv3's epilogue).  C % 4 == 0, 16-byte aligned. */
int dir_bn_train_apply(const float* x, const float* w, const float* b, const float* save_mean, const float* save_rstd, float* y, int R, int C, int ld,
                       int relu, const float* residual, void* stream);
/* dir_bn_train_stats_from_partials (without the affine) + dir_bn_train_apply in one call: dir_bn_train_forward whose statistics pass is replaced by the
 * producing convolution's chunk partials. */
int dir_bn_train_forward_from_partials(const float* x, float* p1, float* p2, int chunk_rows, int cap_rows, const float* w, const float* b, float* y,
                                       float* save_mean, float* save_rstd, float* running_mean, float* running_var, int R, int C, int ld, float eps,
                                       float momentum, int relu, const float* residual, void* stream);
/* BatchNorm with FROZEN statistics inside a training pass (a BatchNorm module put in .eval() under model.train(): torch then normalises with the
 * running statistics and leaves them alone -- torch/nn/modules/batchnorm.py; the reference never freezes them, train.py:64; this form exists
 * because the reference's whole-step gradient is only reproducible (to 4e-5) with it: tests/golden G20e): y = (x - running_mean) / sqrt(running_var
 * + eps) * w + b (+ residual, ReLU as in the training-mode entry points); backward: g w, g b as there, g x = gy w rstd.  save_mean / save_rstd [C]
 * are written by the forward for the backward.  workspace (backward): dir_bn_frozen_workspace_bytes(R, C). */
long long dir_bn_frozen_workspace_bytes(int R, int C);
int dir_bn_frozen_forward(const float* x, const float* w, const float* b, float* y, float* save_mean, float* save_rstd, const float* running_mean,
                          const float* running_var, int R, int C, int ld, float eps, int relu, const float* residual, void* stream);
int dir_bn_frozen_backward(const float* gy, const float* x, const float* w, const float* b, const float* save_mean, const float* save_rstd, float* gx,
                           float* gw, float* gb, int R, int C, int ld, int relu, float* workspace, long long workspace_bytes, void* stream);
/* SyncBN building blocks (round 5; SURVEY.md 8e: the reference trains its batch of 64 on one GPU, config.py:13-15 -- data parallelism over 8 GPUs x 32
 * images changes the BatchNorm batch unless the statistics are pooled; torch.nn.SyncBatchNorm semantics).  The library computes, the caller moves
 * the 2 C (+ 4) floats between the ranks (dir_amd/train/ops.py: all-gather of the parts forward, all-reduce of the sums backward):
 *   dir_bn_sync_local_stats     part [2 C] = this rank's (mean | M2 = sum (x - mean)^2) over its R rows        (the chunked one-pass statistics of
 *                               dir_bn_train_forward);  the caller appends its row count: parts [W][2 C + 4] = (mean | M2 | rows, 0, 0, 0) per rank
 *   dir_bn_sync_combine         pooled mean / BIASED variance [C] from the gathered parts (Chan's exact formula, rank order: identical on every
 *                               rank); running statistics updated with the unbiased variance over the pooled count.  The forward is then
 *                               dir_bn_frozen_forward(x, w, b, y, save_mean, save_rstd, mean, var, ...) -- normalise with GIVEN statistics.
 *   dir_bn_sync_backward_sums   sums [2 C] = this rank's (sum g | sum g xhat), g = gy under the ReLU mask: g b and g w of THIS rank (the data-parallel
 *                               gradient exchange averages them like every other parameter gradient)
 *   dir_bn_sync_backward_apply  g x = w rstd (g - S1 / n - xhat S2 / n) with the sums pooled over all ranks (all-reduce SUM) and n = rows_pooled
 * C and ld multiples of 4, 16-byte aligned pointers; workspace: dir_bn_sync_workspace_bytes(R, C). */
long long dir_bn_sync_workspace_bytes(int R, int C);
int dir_bn_sync_local_stats(const float* x, float* part, int R, int C, int ld, float* workspace, long long workspace_bytes, void* stream);
int dir_bn_sync_combine(const float* parts, int world, int C, float* mean, float* var, float* running_mean, float* running_var, float momentum, void* stream);
int dir_bn_sync_backward_sums(const float* gy, const float* x, const float* w, const float* b, const float* save_mean, const float* save_rstd, float* sums,
                              int R, int C, int ld, int relu, float* workspace, long long workspace_bytes, void* stream);
int dir_bn_sync_backward_apply(const float* gy, const float* x, const float* w, const float* b, const float* save_mean, const float* save_rstd,
                               const float* sums_pooled, float* gx, int R, float rows_pooled, int C, int ld, int relu, void* stream);
int dir_relu_forward(const float* x, float* y, long long n, void* stream);
int dir_relu_backward(const float* gy, const float* y, float* gx, long long n, void* stream);   /* g x = y > 0 ? g y : 0 */
/* Nearest-neighbour upsampling by a power-of-two factor in training form (the fuse layers of an HRNet module, y_i = relu(sum_j f_ij(x_j)) with
 * f_ij = upsample(bn(conv1x1(x_j))) for j > i; no reference counterpart: dir_amd/models/backbone/hrnet.py): dst [B][h f][w f][C] += up(src [B][h][w][C]),
 * and the backward gx [B][h][w][C] = the sum of gy over each f x f block.  NHWC fp32, C % 4 == 0, 16-byte aligned. */
int dir_upsample_nearest_add_f32(const float* src, float* dst, int B, int h, int w, int C, int factor, void* stream);
int dir_upsample_nearest_backward_f32(const float* gy, float* gx, int B, int h, int w, int C, int factor, void* stream);
/* PGraphConv's adjacency (SemGCN/p_graph_conv.py:43-50): A_1 [21][21] = row-softmax of the hand-skeleton mask filled with e_1 [40]
 * (row-major nonzero order); backward: g e_1 from g z [B,21,128] (gradient of the layer's pre-BatchNorm output) and h1 = x W_1 [B,21,128]
 * (g A_1[j][k] = sum_b <g z[b][j], h1[b][k]> on the edges, then the softmax chain rule).  scratch40: 40 floats. */
/* ImgFeature2JointFeature's sampler in training form (models/dir.py:197-198): F.grid_sample(bilinear, zeros, align_corners False) of
 * feat NHWC fp32 [B,S,S,C] at uv [B,21,2] -> rows [B*21][C]; backward w.r.t. feat only (uv arrives detached, models/dir.py:447-453):
 * g feat += sum over `hands` samplers (g_rows_h / uv_h: host arrays of device pointers); zero_first != 0 clears g feat before.
 * Deterministic: the taps of a (sample, channel) are applied in a fixed order by one thread. */
int dir_grid_rows_forward(const float* feat_nhwc, const float* uv, float* rows, int B, int S, int C, void* stream);
int dir_grid_rows_backward(const float* const* g_rows_h_host, const float* const* uv_h_host, int hands, float* g_feat_nhwc, int B, int S, int C,
                           int zero_first, void* stream);
/* Backward pass, image half: the spatial operators between the convolutions (fp32 NHWC, deterministic gather forms).
 * dir_maxpool3x3s2_backward: nn.MaxPool2d(3,2,1) (models/backbone/resnet.py:247): g x from x [B,H,W,C] and g y [B,Ho,Wo,C]; the gradient of a
 *   window goes to its FIRST maximum in (ky, kx) order, as ATen's max_pool2d_with_indices picks it.
 * dir_upsample2x_bilinear_backward: nn.Upsample(2, bilinear) (models/dir.py:392,398): g x [B,H,W,C] from g y [B,2H,2W,*] (channel slice
 *   gy_coff .. +C of rows of gy_cstride floats: the upsampled map is one half of a concatenation).
 * dir_attn_pool_forward / _backward: InitRegressor's pooling (models/dir.py:263-270): attn = sigmoid(logit [B,HW]);
 *   pooled [B,C] = sum_p feat[p,c] attn[p] / (sum_p attn[p] + 1e-8); mean [B,C] = feat.mean over the pixels.  Backward: g feat (written, or
 *   added with accumulate != 0) from g pooled and g mean (either may be NULL), g logit [B,HW] (optional).
 * dir_bone_proj_backward: Joint2BoneFeature.bone_proj (models/dir.py:146-174) for `hands` hands: from g img [B,S,S,*] (channel
 *   (hand*20 + bone)*64 + c at offset img_coff of rows of img_cstride floats) the gradients w.r.t. the re-embedded joint features
 *   emb [B,42,64] (-> g_emb [B,42,64]) and the joint uv [B,21,2] per hand (-> g_uv_lr, optional).  The capsule mask and the weights are
 *   recomputed with the forward's own arithmetic; scratch: dir_bone_proj_backward_scratch_bytes(B, hands). */
int dir_maxpool3x3s2_backward(const float* x, const float* gy, float* gx, int B, int H, int W, int C, void* stream);
int dir_upsample2x_bilinear_backward(const float* gy, float* gx, int B, int H, int W, int C, int gy_cstride, int gy_coff, void* stream);
int dir_attn_pool_forward(const float* feat, const float* logit, float* attn, float* pooled, float* mean, int B, int HW, int C, void* stream);
int dir_attn_pool_backward(const float* feat, const float* attn, const float* pooled, const float* g_pooled, const float* g_mean, float* g_feat,
                           float* g_logit, int B, int HW, int C, int accumulate, void* stream);
long long dir_bone_proj_backward_scratch_bytes(int B, int hands);
int dir_bone_proj_backward(const float* const* uv_lr_host, const float* emb, const float* g_img, int img_cstride, int img_coff, float distance,
                           float* g_emb, float* const* g_uv_lr_host, float* scratch, int B, int S, int hands, void* stream);
/* dst += alpha * src, n floats (gradient accumulation of the modules a stage runs once per hand: global_pos_emb, proj_feat_emb,
 * models/dir.py:106-107,118-119). */
int dir_axpy_f32(float* dst, const float* src, long long n, float alpha, void* stream);
/* dst_t += alpha * src_t for `count` tensors (host arrays of device pointers and element counts) in count / 40 launches: the gradients of a
 * training step into the flat all-reduce bucket (dir_amd/train/step.py::add_grads) */
int dir_axpy_multi_f32(float* const* dst_host, const float* const* src_host, const long long* n_host, int count, float alpha, void* stream);
/* Joint2BoneFeature's token inputs (models/dir.py:97-98,106-107): pos = xyz / 0.15, gpos_left = xyz_left / 0.15 - offset / 2,
 * gpos_right = xyz_right / 0.15 + offset / 2; xyz [B,21,3], offset [B,3], outputs [B*21,3]. */
int dir_stage_positions(const float* xyz_left, const float* xyz_right, const float* offset, float* pos_left, float* pos_right,
                        float* gpos_left, float* gpos_right, int B, void* stream);
int dir_pgcn_adjacency_forward(const float* e1, float* A, void* stream);
int dir_pgcn_adjacency_backward(const float* e1, const float* gz, const float* h1, float* scratch40, float* g_e1, int B, void* stream);

/* ------------------------------------------------------------------------------------------------
 * a1 / a2 / a3 / a11: 2-D convolution as an implicit GEMM on the matrix cores
 * replaces every nn.Conv2d (+ the BatchNorm / bias / ReLU / residual add around it) on the path:
 * models/backbone/resnet.py:120-140,243-255 (Bottleneck, stem excluded), models/backbone/hourglass.py:10-30,
 * 55-70 (Conv, pre-activation Residual), models/dir.py:57-62 (fusion), :227-241 (attention), :404-420 (heads).
 *
 * x  : NHWC activations, B*H*W pixels of in_cstride channels; channels [in_coff, in_coff+Cin) are read
 * w  : [Cout][kh][kw][Cin] in in_dtype  (= torch weight.permute(0,2,3,1))
 * y  : NHWC, out_cstride channels per pixel, channels [out_coff, out_coff+Cout) are written
 *      y = relu?( acc * scale[n] + shift[n] + residual[m][n] )        (scale/shift/residual optional)
 * pre_scale/pre_shift [Cin] (optional): the input is first mapped x -> relu?(x*pre_scale + pre_shift)
 *      (eval-mode BatchNorm+ReLU in front of the conv; zero padding is applied AFTER this map)
 * dtype: in_dtype f32 computes with v_mfma_f32_32x32x2_f32 (exact fp32), bf16 with v_mfma_f32_32x32x16_bf16
 *      (fp32 accumulate).  Cin must be a multiple of 32 (f32) / 64 (bf16); *_cstride = 0 means dense.
 */
#define DIR_DT_F32 0
#define DIR_DT_BF16 1
#define DIR_DT_U8 2 /* input images only (dir_stem_pool_forward) */
/* dir_conv2d_* only, as in_dtype (out_dtype = DIR_DT_F32): "split precision".  Tensors are fp32 in memory; every product a*w is
 * evaluated on the f16 matrix cores as hi(a)*hi(w) + lo(a)*hi(w) + hi(a)*lo(w) with hi(x) = f16(x), lo(x) = f16(x - hi(x)) and fp32
 * accumulation: 22 significant bits per operand (error ~2^-22 |a w| per product, below the fp32 accumulation noise of any K >= 8
 * reduction) at 3 instead of 16 matrix-core cycles per product of the exact fp32 path.  This is the mode that meets the 1e-4 mm parity
 * budget at several times the fp32 mode's speed.  The caller passes the WEIGHTS already split:
 *   w = f16 [Cout][kh][kw][Cin/32][2][32]   (per 32-channel slab: 32 hi values, then the 32 lo values; the same bytes / addressing as
 *                                            the fp32 tensor [Cout][kh][kw][Cin]; for dir_conv2d_dual_* the rows are [kh*kw*Cin | Cin2])
 * of the weights PRE-SCALED per output channel n by a power of two p_n chosen so that max |w_n| p_n lies in [2^12, 2^13) (their lo
 * parts are then normal f16 numbers), with 1 / p_n folded into scale[n] (dir_amd/functional.py::pack_f16x3_weights).  The ACTIVATIONS
 * are split inside the kernel after multiplication by dir_conv_desc.in_scale, a power of two the caller picks per layer so that the
 * layer's typical maximum lands near 2^9 (dir_amd/engine.py::DirEngine.calibrate): 64x headroom below the f16 maximum 65504 (beyond it
 * values saturate), full 22-bit accuracy down to max / 4096, below that an absolute floor of 2^-25 / in_scale per element (f16 denormal
 * lo parts, which the matrix cores honour: tools/ubench_f16_denorm.hip).  Cin % 32 == 0 as for fp32. */
#define DIR_DT_F16X3 3
/* the same operands and packing with the hi parts only: ONE f16 MFMA per product (operands rounded to f16, fp32 accumulation) -- the
 * arithmetic of torch.autocast(float16) on fp32 tensors, 8x finer than bf16; the "fp16 MFMA path" of BASELINE config 5 */
#define DIR_DT_F16X1 4
/* F16X3 / F16X1 with the ACTIVATIONS pre-split as well: x is what dir_split_f16_forward wrote ([pixel][Cin/32][32 hi | 32 lo] f16, the
 * bytes and addressing of an fp32 tensor with in_cstride = Cin, in_coff = 0), already multiplied by in_scale and through the
 * pre-activation (so pre_scale / pre_shift must be NULL here and in_scale is ignored; 1 / in_scale still belongs in scale[]).  Both
 * operands then travel global -> LDS by DMA and nothing is converted per output tile: the form for layers with a long reduction or many
 * output-channel tiles. */
#define DIR_DT_F16X3P 5
#define DIR_DT_F16X1P 6
/* f16 STORAGE (round 5): feature maps and convolution weights held as IEEE binary16 -- byte for byte the layouts, entry points and kernels of
 * DIR_DT_BF16 (64-channel K-slabs, LDS-DMA operand path, v_mfma_f32_32x32x16_f16 instead of _bf16, fp32 accumulation and epilogue), with an
 * 11-bit significand per stored value instead of 8.  Outputs are rounded to nearest even after clamping to +-65504 (no inf is ever stored).
 * Accepted wherever DIR_DT_BF16 is, for the feature-map / convolution-weight side; the token path's weight_dtype / w_dtype stay F32 | BF16. */
#define DIR_DT_F16 7
#define DIR_CONV_RELU 1
#define DIR_CONV_PRE_RELU 2
/* Optional kernel choice in bits 8..15 of dir_conv_desc.flags (0 = the library's per-layer heuristic).  Every variant
 * computes the same fp32 accumulation order (bit-identical results); a variant that does not apply to the layer
 * (alignment, pre-activation, grid) silently falls back to the heuristic.  dir_amd.engine times them per layer.
 *   1..4  : 4-wave kernel (conv.hip), tile 128x128 | 128x64 | 64x128 | 64x64 ; +16: 3-buffer DMA ring
 *   8..10 : 8-wave pipelined kernel (conv_pipe.hip), tile 256x128 | 128x128 | 256x64
 *   11    : 8-wave 256x256 tile, two-deep 64 KB slab ring (conv_big.hip; bf16 operands, Cout > 128, no pre-activation / second source)
 *   12..14: the same tiles with halo reuse (stride-1 kh x kw layers whose tile is a rectangle of image rows)
 *   15    : the 8-wave pipelined kernel on a 128x64 tile (32x32 wave tiles): the small-M layers (8x8 / 16x16 maps)
 *   22, 23: dir_conv1x1_stream_forward only: 64- / 32-pixel workgroups instead of 128 (the 16x16 / 8x8 stages, whose 128-pixel grid does not
 *           cover the CUs); (19 = 64x128 on the ring: not in the product build, see conv.hip)
 *   25..28: dir_conv2d_as_forward only (activation-stationary kernel for the small maps): (A, PB) = (2,2) | (2,4) | (4,2) | (1,2) */
#define DIR_CONV_VARIANT(v) (((v) & 0xff) << 8)

typedef struct dir_conv_desc {
    int32_t B, H, W;
    int32_t Cin, in_cstride, in_coff;
    int32_t Cout, out_cstride, out_coff;
    int32_t res_cstride, res_coff;
    int32_t kh, kw, stride, pad;
    int32_t in_dtype, out_dtype; /* DIR_DT_*; residual is read in out_dtype */
    int32_t flags;               /* DIR_CONV_* */
    int32_t Ho, Wo;              /* 0 = (H + 2*pad - kh)/stride + 1 ; set explicitly for the pre-padded stem image */
    float in_scale;              /* DIR_DT_F16X3 only (0 = 1): a power of two the activations (after the pre-activation, both sources of a
                                    dual convolution) are multiplied by before the f16 hi / lo split, to centre them in the f16 range;
                                    the caller folds 1 / in_scale into scale[].  Scaled values are clamped to +-65504 (no inf / nan). */
    float out_split_scale;       /* 0: y as declared by out_dtype.  != 0 (fp32 outputs that are whole tensors, Cout % 32 == 0): y is written as the pre-split
                                    operand of the NEXT convolution (DIR_DT_F16X3P / F16X1P) instead -- act(result) * |out_split_scale| as f16 hi | lo
                                    slabs (negative: hi only), the same bytes as the fp32 tensor, so that consumer needs no dir_split_f16_forward pass.
                                    |out_split_scale| = the consumer's in_scale. */
} dir_conv_desc;

int dir_conv2d_forward(const dir_conv_desc* desc_host, const void* x, const void* w, const float* scale,
                       const float* shift, const float* pre_scale, const float* pre_shift,
                       const void* residual, void* y, void* stream);
/* round 5 -- dir_conv2d_forward (fp32 output, 16-byte aligned rows) with an output MASK: y = mask > 0 ? (conv(x) + residual) : 0, mask an fp32 tensor laid
 * out like y.  The training step's use: the data gradient of a Bottleneck's conv1 is the gradient of the PREVIOUS block's output, whose ReLU backward
 * (`out = relu(...)`, models/backbone/resnet.py:140) is this mask with that block's stored output -- applied where the gradient is written instead of
 * in a pass of its own over (gradient, output). */
int dir_conv2d_forward_masked(const dir_conv_desc* desc, const void* x, const void* w, const float* scale, const float* shift, const float* pre_scale,
                              const float* pre_shift, const void* residual, const float* mask, void* y, void* stream);
/* round 5 -- the data-gradient convolutions of the training step: dir_conv2d_forward (fp32 output) + residual + output mask (dir_conv2d_forward_masked) + the
 * chunk partials of the BACKWARD pass of the BatchNorm (+ ReLU) whose output's gradient the convolution writes.  y [M][Cout] is d loss / d (BatchNorm
 * output); bn->z [M][Cout] the BatchNorm's input, mean / rstd / w / b [Cout] its saved statistics and affine (w, b may be NULL), relu != 0: the ReLU after it
 * (mask BatchNorm(z) > 0, re-computed like dir_bn_train_backward does).  p1 / p2 [ceil(M / rows)][Cout] (room for ceil(M / 64) x Cout each) receive per M tile
 * the sums of the masked gradient and of the masked gradient times xhat = (z - mean) rstd; *chunk_rows = rows per tile, 0 when the kernel that took the
 * launch does not form them.  Feed them to dir_bn_train_backward_from_partials.  nn.Conv2d <- nn.BatchNorm2d <- nn.ReLU under autograd
 * (models/backbone/resnet.py:125-140, hourglass.py:60-69). */
typedef struct dir_conv_bn_bwd {
    const float *z, *mean, *rstd, *w, *b;
    int32_t relu;
    float *p1, *p2;
} dir_conv_bn_bwd;
int dir_conv2d_forward_ex(const dir_conv_desc* desc, const void* x, const void* w, const float* scale, const float* shift, const float* pre_scale,
                          const float* pre_shift, const void* residual, const float* mask, void* y, const dir_conv_bn_bwd* bn, int* chunk_rows, void* stream);
/* round 5 -- dir_conv2d_forward (no residual, no activation, whole fp32 output tensor) that ALSO forms the chunk partials of the training-mode
 * BatchNorm that follows the convolution (nn.Conv2d -> nn.BatchNorm2d, models/backbone/resnet.py:123-133, hourglass.py:14-27) from the output
 * tile while it is in registers: p1 / p2 [ceil(M / rows)][Cout] (room for ceil(M / 64) x Cout floats each), *chunk_rows = rows (the M tile of the
 * kernel that took the launch: 64 / 128 / 256), or 0 when that kernel does not form them -- then run dir_bn_train_stats on y.  Feed them to
 * dir_bn_train_stats_from_partials. */
int dir_conv2d_forward_stats(const dir_conv_desc* desc, const void* x, const void* w, const float* scale, const float* shift, const float* pre_scale,
                             const float* pre_shift, void* y, float* p1, float* p2, int* chunk_rows, void* stream);

/* fp32 NHWC channel slice x[pixel][in_cstride] (channels [in_coff, in_coff + C)) -> y = the pre-split operand of DIR_DT_F16X3P / F16X1P:
 * v = x (* pre_scale + pre_shift, ReLU if pre_relu: the pre-activation of hourglass.Residual) * in_scale, clamped to +-65504, stored per
 * 32-channel slab as 32 hi = f16(v) then 32 lo = f16(v - hi) (lo = 0 with hi_only).  y: pixels * C * 4 bytes.  C % 32 == 0. */
int dir_split_f16_forward(const float* x, void* y, long long pixels, int C, int in_cstride, int in_coff, const float* pre_scale,
                          const float* pre_shift, int pre_relu, float in_scale, int hi_only, void* stream);

/* The weight operand of DIR_DT_F16X3 (above) from fp32 rows w [N][K] (K % 32 == 0) in one launch, for weights that change every step
 * (training): packed = f16 [N][K/32][2][32], scale_out[n] = (scale_in ? scale_in[n] : 1) / p_n.  Same result as the host packing of
 * dir_amd/functional.py::pack_f16x3_weights (tests/test_gpu_f16x3.py). */
int dir_pack_f16x3_weights(const float* w, void* packed, float* scale_out, const float* scale_in, int N, int K, void* stream);

/* Every convolution weight of one training step in both DIR_DT_F16X3 operand forms, straight from the reference's OIHW parameters
 * (nn.Conv2d.weight, models/backbone/resnet.py:23-40, hourglass.py:14, models/dir.py:58-61) in ONE launch -- the weights change every
 * optimiser step (train.py:70), and packing them per convolution call cost ~600 launches per step.  `table` and `wg_start` live in DEVICE
 * memory.  Per entry: w [Cout][Cin][kh][kw] fp32;
 *   fwd   (may be NULL: skipped)  f16 [Cout][kh*kw*Cin/32][2][32]: rows of the OHWI matrix (k = tap * Cin + c), Cin % 32 == 0;
 *                                 fwd_scale[o] = fwd_inv_in / p_o       (what dir_pack_f16x3_weights returns, times 1 / in_scale)
 *   dgrad (may be NULL: skipped)  f16 [Cin][kh*kw*Cout32/32][2][32]: the transposed convolution's weights, row c, k = tap * Cout32 + o
 *                                 = w[o][c][kh*kw - 1 - tap] (taps flipped, Cout padded to Cout32 = ceil32(Cout) with zeros);
 *                                 dgrad_scale[c] = dgrad_inv_in / p_c.
 * kh * kw must be 1 or 9 and Cin % 4 == 0 (every convolution of the path but the 3-channel stem, which keeps its own packing).
 * wg_start[e] = first workgroup of entry e in the launch grid (workgroups of an entry: Cout if fwd -- one per row --, then Cin / 4 if dgrad --
 * one per four rows), wg_start[entries] = total_workgroups.
 * Bit-identical to dir_pack_f16x3_weights on the copied / flipped / padded matrices (tests/test_gpu_conv_bwd.py). */
typedef struct {
    const float* w; void* fwd; float* fwd_scale; void* dgrad; float* dgrad_scale;
    int32_t Cout, Cin, kh, kw;
    float fwd_inv_in, dgrad_inv_in;
} dir_train_weight;
int dir_train_pack_conv_weights(const dir_train_weight* table, const int* wg_start, int entries, int total_workgroups, void* stream);

/* dir_conv2d_forward with the reduction split over `splits` workgroups per output tile (bf16 -> bf16 layers whose M x Cout grid is too
 * small to fill 256 CUs at the benchmark batch: ResNet layer4 at 8x8, the decoder's 16x16 Residual blocks).  128x128 tiles; every
 * workgroup reduces a contiguous range of K-slabs and writes its raw fp32 partial tile to the workspace; the LAST one to arrive at the
 * tile's counter sums all partials in split order -- so the result does not depend on the arrival order -- and runs the usual epilogue
 * (scale / shift, residual, ReLU).  The summation order differs from the unsplit kernels': outputs agree to bf16 rounding, not bit for
 * bit.  workspace: dir_conv2d_splitk_workspace_bytes(d, splits) bytes, 16-byte aligned, its first 16 KiB ZERO before the first use (the
 * kernel leaves them zero); one workspace must not be shared by launches that can run concurrently.  splits == 1 = dir_conv2d_forward.
 * EXPERIMENTAL, not selected by the engine (functional.conv2d_nhwc(splits=...) calls it): the cross-workgroup hand-over publishes the
 * partial tiles as relaxed
 * agent-scope atomic stores that are drained (s_waitcnt vmcnt(0)) before a relaxed ticket increment -- sufficient on gfx950, where a
 * completed sc1 store is visible device-wide, but NOT a release / acquire pair in the HIP memory model (a formal release on the ticket
 * costs an L2 write-back per workgroup: +12 us per split, which erases the gain).  Measured no faster than the tiled kernels at the
 * benchmark batch; kept for small-batch latency experiments, covered by tests/test_gpu_splitk.py (incl. a many-iteration stress case). */
long long dir_conv2d_splitk_workspace_bytes(const dir_conv_desc* d, int splits);
int dir_conv2d_splitk_forward(const dir_conv_desc* d, const void* x, const void* w, const float* scale, const float* shift,
                              const float* pre_scale, const float* pre_shift, const void* residual, void* y, int splits,
                              void* workspace, long long workspace_bytes, void* stream);

/* d loss / d weight of nn.Conv2d in fp32 (train.py:68 runs autograd through every Conv2d of models/backbone/resnet.py,
 * models/backbone/hourglass.py and models/dir.py): d = the FORWARD geometry (in_cstride / in_coff address x, out_cstride / out_coff address
 * gy), x NHWC [B,H,W,*], gy NHWC [B,Ho,Wo,*], gw [Cout][kh][kw][Cin] (the layout dir_conv2d_forward reads); accumulate != 0 adds to gw.
 * The reduction over the B*Ho*Wo output pixels is cut into chunks whose partial tiles are added in chunk order (deterministic).
 * workspace: dir_conv2d_wgrad_workspace_bytes(d) bytes (0 = none needed unless accumulate, then the weight size).
 * The data gradient needs no kernel of its own: it is dir_conv2d_forward on gy with the flipped, transposed weights (zeros inserted
 * between the rows / columns of gy for stride 2), dir_amd/train/conv.py. */
long long dir_conv2d_wgrad_workspace_bytes(const dir_conv_desc* d);
int dir_conv2d_wgrad_f32(const dir_conv_desc* d, const float* x, const float* gy, float* gw, int accumulate, float* workspace,
                         long long workspace_bytes, void* stream);

/* The same weight gradient on the f16 matrix cores in split precision (the arithmetic of DIR_DT_F16X3: every product gy * x as hi*hi + lo*hi +
 * hi*lo of the operands' f16 hi / lo halves, fp32 accumulation; ~2^-22 per product).  x_scale / gy_scale: powers of two by which x / gy are
 * multiplied before the split (the largest |value| belongs near 2^9 .. 2^10: dir_amd.functional.pow2_in_scale; values saturate at the f16
 * maximum, never inf / nan); 1 / (x_scale * gy_scale) is applied to the result.  Same geometry descriptor, result layout, chunked
 * deterministic pixel reduction and accumulate semantics as dir_conv2d_wgrad_f32; channel counts, strides and offsets must be multiples of 4
 * (DIR_E_ARG otherwise: use dir_conv2d_wgrad_f32).  workspace: dir_conv2d_wgrad_f16x3_workspace_bytes(d). */
long long dir_conv2d_wgrad_f16x3_workspace_bytes(const dir_conv_desc* d);
int dir_conv2d_wgrad_f16x3(const dir_conv_desc* d, const float* x, const float* gy, float* gw, int accumulate, float* workspace,
                           long long workspace_bytes, float x_scale, float gy_scale, void* stream);
/* the same with a pre-activation on the x operand: x <- act(x pre_scale[c] + pre_shift[c]) per input channel (pre_relu != 0: max(., 0)) where the
 * kernel reads it, padding taps zero -- the weight gradient of a convolution whose input is a BatchNorm (+ ReLU) that was never materialised
 * (dir_bn_train_stats).  x_scale is the power-of-two scale of the ACTIVATED operand. */
int dir_conv2d_wgrad_f16x3_pre(const dir_conv_desc* d, const float* x, const float* gy, float* gw, int accumulate, float* workspace,
                               long long workspace_bytes, float x_scale, float gy_scale, const float* pre_scale, const float* pre_shift, int pre_relu,
                               void* stream);

/* A convolution with a SECOND source accumulated into the same output tile:
 *   y = epilogue( conv(x; kh x kw, stride, pad) + conv1x1(x2; stride2) )
 * -- ResNet's projection shortcut (`downsample`, models/backbone/resnet.py:137-140 and :117-119) folded into the block's last
 * convolution, so the identity tensor is neither written nor read back.  w: [Cout][kh*kw*Cin + Cin2] (the second source's
 * columns appended to every row) with both BatchNorm scales pre-multiplied into the rows; shift = the sum of the two folded
 * shifts; flags: DIR_CONV_RELU.  x2: NHWC [B, d2->H, d2->W, in_cstride], read at pixels (oy*stride, ox*stride). */
typedef struct dir_conv_src2 {
    int32_t H, W, Cin, in_cstride, in_coff, stride;
} dir_conv_src2;
int dir_conv2d_dual_forward(const dir_conv_desc* desc, const void* x, const dir_conv_src2* src2, const void* x2, const void* w,
                            const float* shift, void* y, void* stream);
/* the same with a per-output-channel scale applied to the SUM of both sources before the shift (needed by DIR_DT_F16X3, whose weight
 * rows carry a power-of-two prescale; scale may be NULL = dir_conv2d_dual_forward) */
int dir_conv2d_dual_scaled_forward(const dir_conv_desc* desc, const void* x, const dir_conv_src2* src2, const void* x2, const void* w,
                                   const float* scale, const float* shift, void* y, void* stream);

/* The HBM-bound 1x1 convolutions (bf16 in / out, stride 1) as a streaming kernel: small synchronous workgroups (128 pixels x
 * 128 | 256 output channels), several per CU, activations global -> registers -> LDS two K-chunks ahead, weights straight
 * into MFMA operand registers from a stream packed in consumption order.  Same mathematics as dir_conv2d_forward /
 * dir_conv2d_dual_forward for kh = kw = 1 (models/backbone/hourglass.py:55-70 conv1 with its pre-activation and conv3 + skip_layer;
 * models/backbone/resnet.py:117-140 conv1 / conv3 + projection shortcut): y = act(scale * (x . W1^T + x2 . W2^T) + shift), with
 * the optional pre-activation relu(x * pre_scale + pre_shift) on the FIRST source only.  No residual input.
 * desc: kh = kw = stride = 1, pad = 0, Cin % 64 == 0, Cout % 128 == 0, bf16; src2 / x2 optional (1x1, stride src2->stride).
 * w_stream: bf16 [Cout / NWG][4 waves][K / 64 chunks][4 k-steps][NCB][64 lanes][8] with NWG = 256, NCB = 2 when Cout % 256 == 0,
 * else NWG = 128, NCB = 1; lane l of fragment (chunk c, k-step ks, block cb) of wave w in N-chunk g holds
 *   W[g*NWG + (w*NCB + cb)*32 + (l & 31)][64*c + 16*ks + 8*(l >> 5) .. +8],   W = [W1 | W2] along K
 * (dir_amd/engine.py::pack_stream_weights). */
int dir_conv1x1_stream_forward(const dir_conv_desc* desc, const void* x, const dir_conv_src2* src2, const void* x2,
                               const void* w_stream, const float* scale, const float* shift, const float* pre_scale,
                               const float* pre_shift, void* y, void* stream);

/* The convolutions on SMALL maps (W = 8 | 16 | 32, stride 1, 1x1 or 3x3 / pad 1, 16-bit storage in = out) as an ACTIVATION-STATIONARY kernel
 * (conv_as.hip, round 6): a workgroup owns 32 * pixel_blocks pixels of one image (whole rows) x 128 * blocks_per_wave output channels, its whole input
 * patch (every input channel, halo included) goes global -> LDS once by DMA, the weights stream L2 -> MFMA operand registers from a buffer packed in
 * consumption order, and there is no barrier inside the reduction.  Same mathematics, K order and k-slot assignment as dir_conv2d_forward
 * (bit-identical outputs): y = act(scale * conv(x) + shift (+ residual)) -- models/backbone/resnet.py:120-140 (Bottleneck conv1 / conv2 / conv3 +
 * identity at 16x16 and 8x8), models/backbone/hourglass.py:55-70 (Residual conv2), models/dir.py:227-241.  No pre-activation, no second source.
 * (blocks_per_wave A, pixel_blocks PB) in {(2,2), (2,4), (4,2), (1,2)}; Cin % 64 == 0, Cout % (128 A) == 0, (H W) % (32 PB) == 0, (32 PB) % W == 0,
 * patch and staging <= 160 KB of LDS -- or, for (4, 2), a ring of TWO patch chunks of 128 .. 1024 channels (the attention convolution, 8x8x2048:
 * 8 chunks of 256 channels; same K order, bit-identical).  dir_conv2d_as_supported returns 1 when a layer qualifies.
 * w_as: 16-bit [Cout / (128 A)][4 waves][kh kw Cin / 64 steps][4 k-steps][A][64 lanes][8]; step s = (64-channel slab s / (kh kw), tap s % (kh kw)); lane l of
 * fragment (step, ks, cb) of wave w in slice g holds W[g 128 A + (w A + cb) 32 + (l & 31)][tap][64 slab + 8 ks + 32 (l >> 5) .. + 8] of the
 * [Cout][kh][kw][Cin] weights (dir_amd/engine.py::pack_as_weights). */
int dir_conv2d_as_supported(const dir_conv_desc* desc, int blocks_per_wave, int pixel_blocks);
int dir_conv2d_as_forward(const dir_conv_desc* desc, const void* x, const void* w_as, const float* scale, const float* shift,
                          const void* residual, void* y, int blocks_per_wave, int pixel_blocks, void* stream);

/* A 3x3 on the 32x32 map and the 1x1 that is its ONLY reader as one launch (conv_as.hip, the chained mode of the (2, 4) activation-stationary kernel):
 * models/dir.py:474-476 conv_final (3x3 256 -> 256, BN, ReLU, then 1x1 256 -> 256 + bias) and models/dir.py:425-433 the seg / dense heads (3x3, BN, ReLU,
 * then 1x1 -> 3 each; merged: 256 -> 6).  A workgroup owns 128 pixels x all 256 channels of the 3x3, so when its reduction ends it holds everything
 * the 1x1 needs: the 3x3's map is rounded to the storage kind in registers -- t = act(scale * conv3x3(x) + shift), the arithmetic and saturation of
 * dir_conv2d_as_forward's stores -- and kept in LDS as the B operand of a second K = 256 reduction; it never reaches memory.
 *   y[..., out_coff .. + cout2] = act2(scale2 * (t . W2^T) + shift2),   act2 = ReLU when relu2 != 0
 * Same K order and k-slot assignment as dir_conv2d_forward in both reductions: bit-identical to dir_conv2d_as_forward followed by dir_conv2d_forward.
 * desc: the 3x3 (kh = kw = 3, pad 1, stride 1, W = 32, (H W) % 128 == 0, Cin % 64 == 0, Cout = 256, in_dtype = out_dtype = BF16 | F16, DIR_CONV_RELU as
 * wanted; its output slice and residual fields are ignored -- there is no residual).  w_as: pack_as_weights(W, 2) as for dir_conv2d_as_forward.
 * out_dtype = the storage kind: cout2 = 256, w2_as = pack_as_weights(W2 [256][1][1][256], 2), y 16-bit with out_cstride % 8 == out_coff % 8 == 0.
 * out_dtype = DIR_DT_F32: cout2 in {2, 4, 6, 8}, w2_as = pack_as_weights(W2 zero-padded to [128][1][1][256], 1) (only wave 0's share, 16 KB, is read),
 * y fp32 with out_cstride and out_coff even.  out_cstride 0 = cout2.  scale, scale2 (1), shift, shift2 (0) optional.
 * dir_conv2d_as_chain_supported returns 1 when the pair qualifies (no launch); dir_conv2d_as_chain_forward returns DIR_E_INVALID before any launch for
 * whatever it rejects. */
int dir_conv2d_as_chain_supported(const dir_conv_desc* desc, int cout2, int out2_dtype);
int dir_conv2d_as_chain_forward(const dir_conv_desc* desc, const void* x, const void* w_as, const float* scale, const float* shift,
                                const void* w2_as, const float* scale2, const float* shift2, int cout2, int relu2,
                                void* y, int out_cstride, int out_coff, int out_dtype, void* stream);

/* a11 with a10's sparsity: same as dir_conv2d_forward (no prologue), plus group_bbox int32 [B][Cin/64][4] = for every
 * image and every 64-channel input group the pixel box (ymin,ymax,xmin,xmax) outside which that group is exactly zero.
 * K-slabs (tap x group) that cannot touch an output tile are skipped: the sum only loses exact-zero products, so the
 * result is bit-identical to the dense call.  The rasterised bone features (models/dir.py:146-174) are ~93 % zeros and
 * one group == one (hand, bone).  Falls back to dense when (Ho*Wo) % 128 != 0 or Cin % 64 != 0. */
int dir_conv2d_sparse_forward(const dir_conv_desc* desc_host, const void* x, const void* w, const float* scale,
                              const float* shift, const void* residual, void* y, const int32_t* group_bbox,
                              void* stream);

/* ------------------------------------------------------------------------------------------------
 * HBM-bound spatial helpers (NHWC, dtype = DIR_DT_*; arithmetic in fp32)
 */
/* NCHW fp32 image [B,3,H,W] -> zero-padded NHWC4 [B,Hp,Wp,4] (RGB0) with `pad` blank pixels top/left, so that the
 * 7x7/s2 stem (models/backbone/resnet.py:176,244) becomes a kh=7,kw=1 implicit GEMM over contiguous pixel windows. */
int dir_stem_prep(const float* img_nchw, void* out, int B, int H, int W, int Hp, int Wp, int pad, int dtype,
                  void* stream);
/* The same staging as 2x2 space-to-depth blocks: out [B,Hs,Ws,16] (dtype), channel (dy*2+dx)*4 + c =
 * img[b][c][2Y-4+dy][2X-4+dx] (zero outside the image / for c = 3); Hs >= H/2+3, Ws >= W/2+3.  The 7x7/2 stem becomes
 * dir_conv2d_forward with kh=4, kw=1, stride=1, pad=0, Cin=64 (4 blocks x 16 channels), in_cstride=16, Ho=H/2, Wo=W/2 and
 * weights [Cout][4][1][64] (w[n][r][0][j*16 + (dy*2+dx)*4 + c] = conv1.weight[n, c, 2r+dy-1, 2j+dx-1], zero outside 0..6):
 * K = 256 per output instead of 448. */
int dir_stem_prep_s2d(const float* img_nchw, void* out, int B, int H, int W, int Hs, int Ws, int dtype, void* stream);
/* nn.MaxPool2d(3, 2, 1) (models/backbone/resnet.py:179,247): [B,H,W,C] -> [B,(H+1)/2,(W+1)/2,C] */
int dir_maxpool3x3s2(const void* x, void* y, int B, int H, int W, int C, int dtype, void* stream);
/* nn.Upsample(scale_factor=2, mode='bilinear') (models/dir.py:392,398; align_corners=False): [B,H,W,C] ->
 * channels [out_coff, out_coff+C) of y [B,2H,2W,out_cstride] (out_cstride 0 = C) */
int dir_upsample2x_bilinear(const void* x, void* y, int B, int H, int W, int C, int out_cstride, int out_coff,
                            int dtype, void* stream);
/* f4 (HRNet fuse layers; no reference counterpart): acc [B,H,W,C] = act(acc + nearest_upsample(src [B,H/f,W/f,C], f)), in place, one term
 * of `y = y + fuse_layers[i][j](x[j])` at a time; factor 1 = a plain add; relu != 0 on the last term (the fuse layer's ReLU). */
int dir_add_upsampled(void* acc, const void* src, int B, int H, int W, int C, int factor, int relu, int dtype, void* stream);
/* the whole fuse row in one pass (round 5): out [B,H,W,C] = act(base + sum over t < nsrc (<= 4) of nearest_upsample(srcs[t] [B,H/f_t,W/f_t,C], f_t)),
 * summed in fp32 in source order and rounded once; out may be base.  `y = sum_j fuse_layers[i][j](x[j])` + ReLU of an HRNet module (no reference
 * counterpart): 2 passes over the row's map instead of 2 per term + a copy. */
int dir_fuse_sum(void* out, const void* base, const void* const* srcs, const int* factors, int nsrc, int B, int H, int W, int C, int relu, int dtype,
                 void* stream);

/* InitRegressor tail (models/dir.py:263-270): 1x1 conv Ch->1 + sigmoid attention, attention-weighted pooling
 * of c4 (+1e-8), plain mean, Linear C->64 (left, right) and C->3 (offset). */
typedef struct dir_init_head_params {
    const float* attn_w[2]; /* [Ch]    attention_{left,right}.3.weight */
    float attn_b[2];        /*         attention_{left,right}.3.bias   */
    const float* mano_wt;   /* [C][128] k-major: column o < 64 = mano_left.weight[o, :], o >= 64 = mano_right.weight[o-64, :] */
    const float* mano_b[2]; /* [64]                                    */
    const float* off_w;     /* [3][C]  offset.weight                   */
    const float* off_b;     /* [3]                                     */
} dir_init_head_params;
/* c4 [B,HW,C]; h_left/h_right = relu(bn(conv3x3(c4))) of each attention branch (dtype): Ch channels per pixel, pixels
 * h_cstride elements apart (0 = Ch) -- both branches may live in one [B,HW,2*Ch] buffer produced by a single N=2*Ch
 * convolution; outputs fp32: para_left/right [B,64], offset [B,3]. */
int dir_init_head_forward(const dir_init_head_params* params_host, const void* c4, const void* h_left,
                          const void* h_right, int h_cstride, float* para_left, float* para_right, float* offset,
                          int B, int HW, int C, int Ch, int dtype, void* stream);

/* a10: Joint2BoneFeature.bone_proj + lineseg_dists (models/dir.py:132-174) for BOTH hands.
 * uv_left/right [B,21,2] in [-1,1]; emb [B,42,64] (tokens 0..20 left, 21..41 right);
 * out NHWC [B,S,S,2560] (channel = hand*1280 + bone*64 + c == torch.cat((left,right),1) of models/dir.py:122); may be
 * NULL when only vis_nchw is wanted (dir_bone_fusion_forward covers the convolution);
 * vis_nchw (optional) fp32 [B,1280,S,S] = left + right (vis_img_feat / proj_feat, models/dir.py:128,481).
 * The capsule mask `distance < thr` follows the reference's fp32 op order exactly (bit-exact support).
 * group_bbox (optional) int32 [B][40][4]: conservative pixel box (ymin,ymax,xmin,xmax; empty when min > max) outside
 * which channel group hand*20+bone (64 channels) of `out` is exactly zero -- input of dir_conv2d_sparse_forward. */
int dir_bone_proj_forward(const float* uv_left, const float* uv_right, const float* emb, void* out, float* vis_nchw,
                          int32_t* group_bbox, int B, int S, float distance, int dtype, void* stream);

/* ------------------------------------------------------------------------------------------------
 * Joint-token operators of a refinement stage (all fp32)
 */
/* Conv1d(k=1) -> BatchNorm1d(eval) -> ReLU -> Conv1d(k=1) on tokens (models/dir.py:31-56,180-185), weights k-major:
 *   hid = relu((w1t^T x) * s1 + b1)   with s1 = gamma/sqrt(var+eps), b1 = (conv_bias - mean)*s1 + beta
 *   out = w2t^T hid + b2 */
typedef struct dir_token_mlp {
    const float* w1t; /* [Cin][Cmid]  */
    const float* s1;  /* [Cmid]       */
    const float* b1;  /* [Cmid]       */
    const float* w2t; /* [Cmid][Cout] */
    const float* b2;  /* [Cout]       */
} dir_token_mlp;

/* a4 + a12: ImgFeature2JointFeature.forward (models/dir.py:197-200: F.grid_sample bilinear / zeros /
 * align_corners=False at the 21 joint uv, then Conv1d 256->128, BN, ReLU, Conv1d 128->128), pos_emb_{left,right}
 * (xyz/0.15, models/dir.py:97-98) and global_pos_emb (xyz/0.15 -/+ offset/2, models/dir.py:106-107), both hands.
 * feat NHWC [B,S,S,feat_cstride] (feat_dtype), channels [feat_coff, feat_coff+256) are sampled (feat_cstride 0 =
 * dense); uv [B,21,2]; xyz [B,21,3]; offset [B,3];
 * x0   [2][B][21][128] = pos_emb + img2joint (GCN input, models/dir.py:100-101), hand 0 = left
 * gpos [2][B][21][128] = global_pos_emb output. */
int dir_grid_tokens_forward(const void* feat, int feat_dtype, int S, int C, int feat_cstride, int feat_coff,
                            const float* uv_left,
                            const float* uv_right, const float* xyz_left, const float* xyz_right, const float* offset,
                            const dir_token_mlp* img2joint_lr_host, const dir_token_mlp* pos_emb_lr_host,
                            const dir_token_mlp* global_pos_emb_host, float* x0, float* gpos, int B, void* stream);

/* a5: one _GraphConv = PGraphConv + BatchNorm1d(eval) + ReLU (SemGCN/p_graph_conv.py:39-59, SemGCN/p_gcn.py:20-27) */
typedef struct dir_pgcn_layer {
    const float* W;        /* gconv.W: w_dtype DIR_DT_F32 -> fp32 [2][21][128 k][128 o] (reference layout, exact fp32 MFMA);
                              DIR_DT_BF16 -> bf16 [2][21][128 o][128 k] (transposed), bf16 MFMA with fp32 accumulation =
                              torch.autocast semantics for the two matmuls of SemGCN/p_graph_conv.py:47-48            */
    const float* e1;       /* [40]               gconv.e_1, row-major nonzero order of adj > 0    */
    const float* bias;     /* [128]              gconv.bias                                       */
    const float* bn_scale; /* [128]              gamma / sqrt(var + eps)                          */
    const float* bn_shift; /* [128]              beta - mean * bn_scale                           */
    int32_t relu;          /* 1: ReLU after BN (the _GraphConv of the network); 0: bare PGraphConv (scale 1, shift 0) */
    int32_t w_dtype;       /* DIR_DT_F32 | DIR_DT_BF16 (layout of W above)                                              */
} dir_pgcn_layer;
/* ResSimplePGCN.forward (SemGCN/p_gcn.py:71-73): x [B,21,128] -> out; `add` (optional, [B,21,128]) is added after the
 * last layer (global_pos_emb, models/dir.py:109-110); out rows are out_bstride floats apart so both hands can write
 * into one [B,42,128] token buffer.  e_0 is a dead parameter (softmax of a diagonal-only mask == I). scratch: 2*B*21*256
 * floats. */
int dir_pgcn_stack_forward(const dir_pgcn_layer* layers_host, int num_layers, const float* x, const float* add,
                           float* out, long long out_bstride, float* scratch, int B, void* stream);

/* both hands in one launch sequence: x_lr / add_lr [2][B][21][128] (hand 0 = left), tokens [B][42][128] (left tokens
 * 0..20, right 21..41), scratch 4*B*21*256 floats. */
int dir_pgcn_stack_forward_pair(const dir_pgcn_layer* layers_left_host, const dir_pgcn_layer* layers_right_host,
                                int num_layers, const float* x_lr, const float* add_lr, float* tokens, float* scratch,
                                int B, void* stream);

/* a6: STE.forward (transformer/mixSTE.py:194-205) on [B,42,128] -> [B,42,64].
 * weight_dtype DIR_DT_F32: the six Linear weights per block (*_wt) and head_wt are fp32, k-major ([in][out]); exact fp32.
 * weight_dtype DIR_DT_BF16: they are bf16 in nn.Linear's own [out][in] layout and the Linears run on the bf16 matrix cores
 * with fp32 accumulation -- torch.autocast(bfloat16) semantics (BASELINE config 4); LayerNorm, softmax, attention and the
 * residual stream stay fp32, biases and LayerNorm parameters are fp32 in both modes. */
typedef struct dir_ste_block {
    const float *ln1_w, *ln1_b, *qkv_wt, *qkv_b, *proj_wt, *proj_b, *ln2_w, *ln2_b, *fc1_wt, *fc1_b, *fc2_wt, *fc2_b;
} dir_ste_block;
typedef struct dir_ste_params {
    const float* pos_embed;  /* [42][128] */
    dir_ste_block blocks[3]; /* STEblocks[1..3]: block 0 is never executed (transformer/mixSTE.py:197) */
    int32_t num_blocks;      /* depth - 1 */
    const float *snorm_w, *snorm_b, *head_ln_w, *head_ln_b, *head_wt /* [128][64] */, *head_b;
    int32_t weight_dtype;    /* DIR_DT_F32 | DIR_DT_BF16 */
} dir_ste_params;
/* x_pos_out (optional): receives x + pos_embed, reproducing the reference's in-place `x += pos` on its input. */
int dir_ste_forward(const dir_ste_params* params_host, const float* x, float* x_pos_out, float* y, int B,
                    void* stream);

/* a7 + a12: RegressorOffset Linears (models/dir.py:342-351) + proj_feat_emb (models/dir.py:118-119).
 * tok [B,42,64]; prev_para_* [B,64] (detached previous mano_para); prev_offset [B,3];
 * para_* [B,64] = Linear(cat(tok_hand.flatten(), prev_para)), offset [B,3] = Linear(cat(tokL, tokR, prev_offset)),
 * emb [B,42,64] = proj_feat_emb(tok). */
typedef struct dir_regress_params {
    const float* mano_wt;   /* [1408][128] k-major: column o < 64 = regressor.mano_left.weight[o, :],
                               o >= 64 = regressor.mano_right.weight[o - 64, :]                       */
    const float* mano_b[2]; /* [64]                                          */
    const float* off_w;     /* [3][2691]  regressor.offset.weight            */
    const float* off_b;     /* [3]                                           */
    dir_token_mlp emb;      /* 64 -> 64 -> 64                                */
} dir_regress_params;
int dir_regress_forward(const dir_regress_params* params_host, const float* tok, const float* prev_para_left,
                        const float* prev_para_right, const float* prev_offset, float* para_left, float* para_right,
                        float* offset, float* emb, int B, void* stream);

/* a10 + a11 fused (bf16 throughput mode): Joint2BoneFeature.bone_proj (models/dir.py:132-174) + fusion[0..2] (3x3 conv
 * 2560 -> 256 + BatchNorm + ReLU, models/dir.py:57-62) without the [B,S,S,2560] bone map.  The rasterised operand is rank 2
 * per bone, so conv(img)[p,n] = sum_tap sum_e Wgt[p+tap, e] * G[tap, e, n] with e = (hand, bone, end) in [0,80),
 * G[tap,(hb,end),n] = sum_c f_end[hb][c] * W[n, hb*64+c, tap] and Wgt = mask * (wa | wb): K = 720 instead of 23040.
 * Same mathematics as dir_bone_proj_forward + dir_conv2d_forward, re-associated (so the fp32 parity mode keeps those).
 * Two launches so that the first can overlap the MANO layer (it needs the token features only):
 *   dir_bone_fusion_prepare : G for every sample from emb [B,42,64] (proj_feat_emb output) into `scratch`
 *                             (dir_bone_fusion_scratch_bytes(B) bytes of device memory);
 *   dir_bone_fusion_forward : uv_* [B,21,2] (pd_joint_uv) + scratch -> y, NHWC bf16 (fp32 with exact_f32) [B,S,S,out_cstride],
 *                             channels [out_coff, out_coff+256).  S in {16, 32, ...} with 256 % S == 0 and S*S % 256 == 0
 *                             (exact_f32: 128 % S == 0). */
typedef struct dir_bone_fusion_params {
    const float* w_g;   /* [9][40][64][256]: fusion.0.weight[n, hb*64 + c, ky, kx] at [ky*3+kx][hb][c][n], rounded to bf16 */
    const float* scale; /* [256] folded fusion.1 BatchNorm scale            */
    const float* shift; /* [256] folded BatchNorm shift (+ fusion.0 bias)   */
    int32_t exact_f32;  /* 0: bf16 operands (w_g rounded to bf16 by the caller, G and Wgt rounded to bf16, y bf16) -- the throughput mode;
                           1: everything fp32 on the exact fp32 matrix cores (w_g unrounded, y NHWC fp32) -- the parity modes: differs from
                           bone_proj + conv3x3 only by the association of the sum (fp32 rounding noise);
                           2 (round 5): as 0 with f16 instead of bf16 everywhere (w_g rounded to f16 by the caller, G / Wgt / y f16: DIR_DT_F16)      */
    float g_scale;      /* exact_f32 only.  0: the exact fp32 matrix cores.  A power of two > 0: split precision on the f16 matrix cores (the
                           arithmetic of DIR_DT_F16X3: hi*hi + lo*hi + hi*lo per product, ~2^-22) -- G is multiplied by g_scale before its f16
                           hi / lo split (the largest |G| belongs near 2^9 .. 2^10: DirEngine.calibrate; values saturate, never inf / nan)      */
} dir_bone_fusion_params;
size_t dir_bone_fusion_scratch_bytes(int B);
int dir_bone_fusion_prepare(const dir_bone_fusion_params* params_host, const float* emb, void* scratch, int B, void* stream);
int dir_bone_fusion_forward(const dir_bone_fusion_params* params_host, const float* uv_left, const float* uv_right,
                            const void* scratch, void* y, int B, int S, float distance, int out_cstride, int out_coff,
                            int relu, void* stream);
/* Backward of the factorised form for the training step (reference: torch autograd through models/dir.py:132-174 and the
 * first convolution of `fusion`, models/dir.py:57-62, run by train.py:66-70).  Forward of the training path = dir_bone_fusion_prepare +
 * dir_bone_fusion_forward with exact_f32 = 1, g_scale = 0, scale = NULL, shift = fusion.0.bias, relu = 0 (the raw convolution; BatchNorm
 * with batch statistics follows as its own step).  From gy [B,S,S,256] (NHWC fp32, contiguous):
 *   g_w_g  [9][40][64][256]   gradient of w_g (the caller permutes it back to fusion.0.weight's OIHW);
 *   g_emb  [B,42,64]          gradient of the re-embedded joint features (both the G path and index_select's backward);
 *   g_uv_* [B,21,2]           gradient of the stage's joint uv through the bone weights (optional, NULL to skip);
 * g_scratch = the G that dir_bone_fusion_prepare(exact_f32 = 1) wrote for this batch.  No [B,S,S,2560] map or gradient map exists:
 * four groups of exact-fp32 GEMMs (dir_gemm_f32) over zero-bordered pixel grids in which a tap is a pointer shift (csrc/bonefuse_bwd.hip).
 * Deterministic.  workspace: dir_bone_fusion_backward_workspace_bytes(B, S) bytes, 16-byte aligned. */
long long dir_bone_fusion_backward_workspace_bytes(int B, int S);
int dir_bone_fusion_backward(const float* w_g, const float* emb, const float* uv_left, const float* uv_right, const void* g_scratch,
                             const float* gy, float distance, float* g_w_g, float* g_emb, float* g_uv_left, float* g_uv_right,
                             void* workspace, long long workspace_bytes, int B, int S, void* stream);

/* ---- evaluation-metric maths of apps/eval.py --------------------------------------------------
 * f1a: Jr.__call__ (apps/eval.py:43-44): joints[B,21,3] = jr[21,778] @ verts[B,778,3].  `jr` is the Jr-processed
 * regressor (16 MANO rows + 5 one-hot fingertip rows, re-ordered; built on the host by dir_amd.apps.eval.Jr).
 * Dot products accumulate in fp64 and round once to fp32. */
int dir_joint_regress_forward(const float* jr, const float* verts, float* joints, int B, void* stream);

/* f1b: the per-batch body of the eval loop, apps/eval.py:151-241, for both hands (index 0 = left, 1 = right).
 * Inputs (device, fp32, contiguous): verts_pd[h] [B,778,3] = result[-1]['pd_mesh_xyz_*'] (:171-172), pd_offset [B,3]
 * (:170, multiplied by 0.15 inside), verts_gt[h] [B,778,3] = data[3]/data[5] (camera space), verts2d_gt[h] [B,778,2] =
 * data[7]/data[9], cam [B,3,3] = data[10], jr[h] [21,778].
 * Outputs (any may be NULL): joint_err/joint2d_err [B,2,21], vert_err/vert2d_err [B,2,778] (:192,204,217,225: L2 norms,
 * metres / pixels), joints_pd/joints_gt [B,2,21,3] (:195-196: aligned prediction, root-relative GT), root_err [B]
 * (:233-239).  root_joint = opt.root_joint (0 wrist | 9 middle MCP), use_scale = opt.scale (:180-185). */
typedef struct dir_eval_inputs {
    const float* verts_pd[2];
    const float* pd_offset;
    const float* verts_gt[2];
    const float* verts2d_gt[2];
    const float* cam;
    const float* jr[2];
} dir_eval_inputs;
typedef struct dir_eval_outputs {
    float *joint_err, *vert_err, *joint2d_err, *vert2d_err, *joints_pd, *joints_gt, *root_err;
} dir_eval_outputs;
int dir_eval_metrics_forward(const dir_eval_inputs* in_host, const dir_eval_outputs* out_host, int B, int root_joint,
                             int use_scale, void* stream);

/* f1d: the validation metric of the training loop, InterHandDataset.evaluate (dataset/interhand.py:262-315) for every stage of a
 * batch, accumulated as Trainer.test_model does (train.py:157-181).  Root = MANO joint 9 of pd_joint_xyz_* / joint_3d_* (no joint
 * regression, whatever the model's root_joint), scale = |J9 - J0|_gt / |J9 - J0|_pred per hand and sample, errors = L2 norms of
 * (pred - root_pred) * scale - (gt - root_gt) in fp32.  Hand index 0 = left, 1 = right; all inputs device fp32, contiguous:
 * joints_pd[s][h] [B,21,3] / verts_pd[s][h] [B,778,3] = outs_list[s]['pd_joint_xyz_*' / 'pd_mesh_xyz_*'] for s < n_stages (1..8),
 * joints_gt[h] / verts_gt[h] = targets['joint_3d_*' / 'mesh_3d_*'].
 * sample_sums: double [n_stages][B][4] scratch the caller owns; on return (of the stream) it holds every sample's sums of norms
 * (joint L, joint R, vert L, vert R; metres).  acc: double [n_stages][4], batches: long long [1]: the caller's running sums; each
 * call ADDS the batch means in millimetres (sum / (B * 21 | 778) * 1000) to acc and 1 to *batches, in a fixed order (no atomics: the
 * same calls give the same bits).  MPJPE_s left = acc[s][0] / *batches, and so on.  A predicted bone of length 0 gives inf / NaN as in
 * the reference.  B = 0 is a no-op.  Two launches, no host synchronisation, nothing allocated. */
#define DIR_VAL_MAX_STAGES 8
typedef struct dir_val_metrics_desc {
    const float* joints_pd[DIR_VAL_MAX_STAGES][2];
    const float* verts_pd[DIR_VAL_MAX_STAGES][2];
    const float* joints_gt[2];
    const float* verts_gt[2];
    double* sample_sums;
    double* acc;
    long long* batches;
} dir_val_metrics_desc;
int dir_val_metrics_forward(const dir_val_metrics_desc* desc_host, int n_stages, int B, void* stream);

/* f1c: the ground-truth MANO layer, models/manolayer.py:251-323 (ManoLayer.forward; rodrigues_batch :32-48), the
 * formulation dataset/interhand.py:130-149 uses to synthesise GT.  Tables in the dir_mano_tables packing (comps = the full
 * [45][45] hands_components, the first `ncomps` rows are used; side / root_palm are ignored: fingertip vertices are
 * 745,317,444,556,673 for both hands, models/manolayer.py:297).  root_rotation [B,3,3]; pose [B,ncomps] PCA coefficients
 * (use_pca) or, with ncomps = 0, [B,15,3,3] rotation matrices; shape [B,10]; trans [B,3] / scale [B] optional (NULL);
 * center_idx -1 = None; verts [B,778,3], joints [B,21,3] (metres). */
int dir_gt_mano_forward(const dir_mano_tables* tables_host, const float* root_rotation, const float* pose, int ncomps,
                        const float* shape, const float* trans, const float* scale, int center_idx, int new_skel,
                        float* verts, float* joints, int B, void* stream);

/* f3 (tensor side of the input pipeline): apps/eval.py:59-61 == dataset/interhand.py:223-225 --
 * uint8 BGR HWC [B,H,W,3] (what cv.imread / cv.resize hand over) -> RGB, / 255, (t - mean) / std -> fp32 NCHW [B,3,H,W],
 * in the reference's fp32 operation order (bit-identical to the torch CPU result).  mean / std: host pointers to 3 floats
 * (ImageNet: 0.485 0.456 0.406 / 0.229 0.224 0.225).  JPEG decode and resize stay on the host. */
int dir_image_normalize_forward(const uint8_t* img_bgr_hwc, float* out_nchw, const float* mean_host, const float* std_host,
                                int B, int H, int W, void* stream);
/* the same arithmetic fused into the space-to-depth stem staging (== dir_image_normalize_forward + dir_stem_prep_s2d,
 * bit for bit, without the fp32 image in HBM) */
int dir_stem_prep_s2d_u8(const uint8_t* img_bgr_hwc, void* out, const float* mean_host, const float* std_host, int B, int H,
                         int W, int Hs, int Ws, int dtype, void* stream);

/* a1 (stem), bf16 mode: models/backbone/resnet.py:244-247 -- conv1 7x7/s2/p3 (3->64) + bn1 (eval, folded scale / shift) + ReLU +
 * MaxPool2d(3,2,1) in ONE launch; with uint8 input also apps/eval.py:59-61 (== dir_image_normalize_forward, bit for bit).
 * img: DIR_DT_F32 -> fp32 NCHW [B,3,H,W] (normalised), DIR_DT_U8 -> uint8 BGR HWC [B,H,W,3] (mean / std: host pointers to 3
 * floats, else ignored).  w_packed: bf16 [64][7 ky][8 kx][4 c] = conv1.weight[n][c][ky][kx], zero for kx = 7 and c = 3.
 * y: bf16 NHWC [B,H/4,W/4,64].  H, W multiples of 4.  Same operand rounding as dir_stem_prep_s2d + dir_conv2d_forward +
 * dir_maxpool3x3s2 (bf16 operands, fp32 accumulation, bf16 conv output); only the summation order inside K differs. */
int dir_stem_pool_forward(const void* img, int img_dtype, const float* mean_host, const float* std_host, const void* w_packed,
                          const float* scale, const float* shift, void* y, int B, int H, int W, void* stream);
/* the same with the 16-bit storage kind of y and w_packed chosen by the caller: out_dtype DIR_DT_BF16 (what the entry point above passes) or
 * DIR_DT_F16 (round 5: f16 feature maps and weights, v_mfma_f32_16x16x32_f16) */
int dir_stem_pool_forward_dt(const void* img, int img_dtype, int out_dtype, const float* mean_host, const float* std_host, const void* w_packed,
                             const float* scale, const float* shift, void* y, int B, int H, int W, void* stream);

/* a1 (layer1 bottlenecks), bf16 mode: models/backbone/resnet.py:126-140 of block i -- conv2 3x3/s1/p1 (64->64) + bn2 + ReLU +
 * conv3 1x1 (64->256) + bn3 + identity + ReLU -- and, optionally, :122-124 of block i+1 -- conv1 1x1 (256->64) + bn1 + ReLU --
 * in one launch: the 64-channel intermediate and the next conv1's input never touch HBM (534 -> 334 MB per block at B = 64).
 * y1 [B,H,W,64] = ReLU(bn1(conv1(x))) of block i; residual [B,H,W,256] or NULL; out [B,H,W,256]; y1_next [B,H,W,n_next] or NULL
 * (then w1n / scale1n / shift1n are ignored); all bf16 NHWC.  H % 8 == 0, W % 16 == 0.  Weights bf16: w2 [64][3][3][64]
 * (dir_conv2d_forward's packing), w3 [256][64], w1n [64][256]; scale / shift = folded eval BatchNorm, fp32, device pointers.
 * Same rounding points as the unfused dir_conv2d_forward sequence (bf16 operands, fp32 accumulation, bf16 y2 / out). */
typedef struct dir_bneck_chain_params {
    const void* w2; const float* scale2; const float* shift2;
    const void* w3; const float* scale3; const float* shift3;
    const void* w1n; const float* scale1n; const float* shift1n;
    const void* wd;   /* projection shortcut (models/backbone/resnet.py:117-119), bf16 [256][64]: with x2 != NULL conv3's GEMM gets
                         64 more K from x2 [B,H,W,64] (the block input).  Both BatchNorm scales must then be folded into w3 / wd
                         rows, scale3 = 1 and shift3 = shift_bn3 + shift_bn_ds; `residual` must be NULL. */
    int32_t n_next;   /* output channels of the fused next conv1: 64 (next layer1 block) or 128 (layer2's first block); y1_next is
                         [B,H,W,n_next], w1n [n_next][256] */
    int32_t out_decimate; /* 0: out is [B,H,W,256].  1: only the pixels with even y and even x are written, as out [B,H/2,W/2,256] -- for the last
                         layer1 block, whose output is read by layer2's stride-2 projection shortcut alone (models/backbone/resnet.py:117-119;
                         its conv1 is the fused y1_next): three quarters of the 256-channel map never leave the CU.  The ResNet's c1 feature is
                         then not produced (models/dir.py never reads it: models/dir.py:437-483 use c2..c4) */
    int32_t dtype;    /* storage kind of every 16-bit tensor and weight of the call: 0 or DIR_DT_BF16 -> bf16, DIR_DT_F16 -> f16 (round 5) */
} dir_bneck_chain_params;
int dir_bottleneck_chain_forward(const dir_bneck_chain_params* p, const void* y1, const void* residual, const void* x2, void* out,
                                 void* y1_next, int B, int H, int W, void* stream);

/* a1, layer2 / layer3 geometry (planes P = 128 | 256): the 1x1 TAIL of a bottleneck and the 1x1 HEAD of the next one in one launch
 *   models/backbone/resnet.py:132-140   out = relu(bn3(conv3(y2)) + identity)            conv3: 1x1, P -> 4P
 *   models/backbone/resnet.py:122-124   y1_next = relu(bn1'(conv1'(out)))                conv1': 1x1, 4P -> n_next
 * bf16 NHWC: y2 [M][P], residual [M][4P] (the block input), out [M][4P], y1_next [M][n_next]; M = B*H*W pixels, a multiple of 64
 * (1x1 convolutions: the image geometry does not matter).  The block output is written once and never read back.
 * wstream: both weight matrices as bf16 MFMA A-operand fragments in the order the kernel's waves consume them (16 bytes per lane,
 * 1 KB per fragment), [4P/512 halves][8 waves][NBF + NCF fragments][64 lanes][8 bf16]:
 *   conv3 fragment f < NBF = P/8        channel block cb = f / (P/16), k-step ks = f % (P/16): lane l holds
 *                                       w3[half*512 + 64*wave + 32*cb + (l & 31)][16*ks + 8*(l >> 5) .. +8]
 *   conv1' fragment fc (n_next = 256)   NCF = 32: w1n[32*wave + (l & 31)][half*512 + 16*fc + 8*(l >> 5) .. +8]
 *   conv1' fragment fc (n_next = 128)   NCF = 16: w1n[16*wave + (l & 15)][half*512 + 32*fc + 8*(l >> 4) .. +8]
 * (dir_amd/engine.py::pack_tail_stream builds it).  scale / shift: the folded eval-mode BatchNorms, fp32. */
typedef struct dir_bneck_tail_params {
    const void* wstream;
    const float* scale3; const float* shift3;      /* [4P]     */
    const float* scale1n; const float* shift1n;    /* [n_next] */
    int32_t planes;   /* P: 128 | 256 */
    int32_t n_next;   /* 128 | 256 (P = 128), 256 (P = 256) */
    int32_t waves;    /* 8: the layout above (64-pixel tiles, one workgroup per CU).  4: the thin variant (32-pixel tiles, two
                         workgroups per CU, for M <~ 64 pixels x CUs): [halves][4 waves][P/4 + 32*(n_next/128) fragments][64][8] with
                         conv3 fragment f < P/4: cb = f / (P/16), ks = f % (P/16): w3[half*512 + 128*wave + 32*cb + (l&31)][16*ks + 8*(l>>5)..],
                         conv1' fragment fc: ks = fc / (n_next/128), cc = fc % (n_next/128):
                         w1n[(n_next/4)*wave + 32*cc + (l&31)][half*512 + 16*ks + 8*(l>>5)..] */
    int32_t dtype;    /* storage kind of the tensors and of the weight stream: 0 or DIR_DT_BF16 -> bf16, DIR_DT_F16 -> f16 (round 5) */
} dir_bneck_tail_params;
int dir_bottleneck_tail_forward(const dir_bneck_tail_params* p, const void* y2, const void* residual, void* out, void* y1_next,
                                long long M, void* stream);

/* a1, decoder: one hourglass Residual block with a projection skip in ONE launch (csrc/res_chain.hip)
 *   models/backbone/hourglass.py:33-70   out = conv3(relu(bn3(conv2(relu(bn2(conv1(relu(bn1(x)))))))) + skip_layer(x)
 * for the shape four of the decoder's six blocks have: Cin = 512, Cmid = 128, Cout = 256, stride 1, on 32x32 or 16x16 maps, 16-bit storage
 * (DIR_DT_BF16 | DIR_DT_F16).  x is NHWC [B,H,W,in_cstride] read from channel in_coff; out is NHWC [B,H,W,out_cstride] written at channels
 * [out_coff, out_coff + 256), every other channel of the buffer is left alone.  y1 and y2 stay on the CU.  Same fp32 accumulation chains and
 * rounding points (y1, y2 and out rounded to the storage kind) as dir_conv2d_forward (conv1 with the pre-activation) -> dir_conv2d_forward
 * (conv2) -> dir_conv2d_dual_forward (conv3 + skip_layer): the output is bit-identical to those three launches.
 * w1 / w2 / w3: the three weight matrices as MFMA A-operand fragments in the order the kernel's waves consume them, the layout of
 * dir_conv2d_as_forward's weight stream with one 32-channel block per wave (dir_amd/engine.py::pack_as_weights(w, 1)):
 *   [Cout / 128][4][steps][4 k-steps][64 lanes][8], step = (64-channel slab) * (kh kw) + tap; lane l of k-step ks holds
 *   W[32 * block + (l & 31)][tap * Cin + 64 * slab + 8 * ks + 32 * (l >> 5) .. + 8]
 * from conv1.weight [128][512], conv2.weight [128][3][3][128] and [conv3.weight | skip_layer.weight] [256][128 + 512].
 * pre_scale / pre_shift [512]: bn1 folded; scale1 / shift1 [128]: bn2 (+ conv1 bias) folded; scale2 / shift2 [128]: bn3 (+ conv2 bias);
 * shift3 [256]: conv3 bias + skip_layer bias.  fp32 device pointers.
 * dir_residual_chain_supported: 1 if the forward call takes these shapes, else 0 (the caller then runs the three launches); no launch.
 * dir_residual_chain_forward returns DIR_E_INVALID for anything dir_residual_chain_supported rejects. */
typedef struct dir_res_chain_params {
    const void* w1; const void* w2; const void* w3;
    const float* pre_scale; const float* pre_shift;
    const float* scale1; const float* shift1;
    const float* scale2; const float* shift2;
    const float* shift3;
    int32_t Cin, Cmid, Cout;   /* 512, 128, 256 */
    int32_t dtype;             /* DIR_DT_BF16 | DIR_DT_F16: storage kind of x, out and the weight streams */
} dir_res_chain_params;
int dir_residual_chain_supported(int dtype, int Cin, int Cmid, int Cout, int B, int H, int W, int in_cstride, int in_coff, int out_cstride,
                                 int out_coff);
int dir_residual_chain_forward(const dir_res_chain_params* p, const void* x, void* out, int B, int H, int W, int in_cstride, int in_coff,
                               int out_cstride, int out_coff, void* stream);

/* a1, layer3 geometry (planes 256, block width 1024, 16-wide maps; ABI 55; csrc/l3_chain.hip): one identity bottleneck from conv2 on, and the
 * 1x1 head of the next one, in ONE launch
 *   models/backbone/resnet.py:126-130   y2 = relu(bn2(conv2(y1)))                          conv2: 3x3 / s1 / p1, 256 -> 256; y2 stays on the CU
 *   models/backbone/resnet.py:132-140   out = relu(bn3(conv3(y2)) + identity)              conv3: 1x1, 256 -> 1024
 *   models/backbone/resnet.py:122-124   y1_next = relu(bn1'(conv1'(out)))                  conv1': 1x1, 1024 -> n_next (n_next = 256; 0: none)
 * 16-bit NHWC, contiguous: y1 [B,H,16,256], residual [B,H,16,1024] (the block input), out [B,H,16,1024], y1_next [B,H,16,256] (ignored when
 * n_next = 0).  W = 16, H a multiple of 4: a workgroup owns four whole rows of one image.  out and y1_next are the only memory written.
 * Bit-identical to dir_conv2d_as_forward (conv2) followed by dir_bottleneck_tail_forward (n_next = 256) or by conv3 as dir_conv2d_forward with
 * the residual (n_next = 0): same fp32 chains, same rounding points (y2, out and y1_next rounded to the storage kind).
 * wstream: the three weight matrices as MFMA A-operand fragments (16 bytes per lane, 1 KB per fragment) in the order the kernel's 8 waves consume
 * them, [8 waves][144 + 2 (32 + NCF) fragments][64 lanes][8], NCF = 32 (n_next = 256) | 0; for wave w, lane l:
 *   conv2 fragment f < 144          step = f / 4 = (64-channel slab) * 9 + tap, ks = f % 4 (dir_conv2d_as_forward's stream with one block per wave):
 *                                   w2[32 w + (l & 31)][tap][64 slab + 8 ks + 32 (l >> 5) .. + 8]
 *   then per 512-channel half: 32 conv3 fragments (channel block cb = f / 16, k-step ks = f % 16) and NCF conv1' fragments fc
 *     n_next = 256                  w3[half 512 + 64 w + 32 cb + (l & 31)][16 ks + 8 (l >> 5) .. + 8]        (dir_bottleneck_tail_forward's stream)
 *                                   w1n[32 w + (l & 31)][half 512 + 16 fc + 8 (l >> 5) .. + 8]
 *     n_next = 0                    w3[half 512 + 64 w + 32 cb + (l & 31)][64 (ks / 4) + 8 (ks % 4) + 32 (l >> 5) .. + 8]   (a convolution's k-slots)
 * (dir_amd/packing.py::pack_l3_stream builds it).  scale / shift: the folded eval-mode BatchNorms, fp32 device pointers.
 * dir_bottleneck_block_supported: 1 if the forward call takes these shapes, else 0 (the caller then runs the two launches); no launch.
 * dir_bottleneck_block_forward returns DIR_E_INVALID for anything dir_bottleneck_block_supported rejects, before any launch. */
typedef struct dir_bneck_block_params {
    const void* wstream;
    const float* scale2; const float* shift2;      /* [256]  */
    const float* scale3; const float* shift3;      /* [1024] */
    const float* scale1n; const float* shift1n;    /* [n_next], or NULL with n_next = 0 */
    int32_t planes;   /* 256 */
    int32_t n_next;   /* 256 | 0 */
    int32_t dtype;    /* DIR_DT_BF16 | DIR_DT_F16: storage kind of the tensors and of the weight stream */
} dir_bneck_block_params;
int dir_bottleneck_block_supported(int dtype, int planes, int n_next, int B, int H, int W);
int dir_bottleneck_block_forward(const dir_bneck_block_params* p, const void* y1, const void* residual, void* out, void* y1_next,
                                 int B, int H, int W, void* stream);

/* a13 / 8f rank 2, forward half: the training objective, models/dir.py:542-594 (SmoothL1Loss models/loss.py:63-93, EdgeLengthLoss
 * :36-60, NormalVectorLoss :6-33, nn.CrossEntropyLoss(weight), lovasz_softmax models/lovasz_loss.py:155-202).  Forward values;
 * the gradients w.r.t. the predictions are dir_stage_losses_backward / dir_dense_losses_backward below.  All tensors fp32, device pointers, index 0 = left hand, 1 = right hand. */
typedef struct dir_loss_pred {      /* one entry of iter_outs (models/dir.py:519,571) */
    const float* joint_uv[2];       /* pd_joint_uv_*  [B,21,2] */
    const float* mesh_uv[2];        /* pd_mesh_uv_*   [B,778,2] (dir_mano_forward's optional output), or NULL: then computed here */
    const float* proj[2];           /* pd_proj_* [B,3] = (scale, tx, ty): mesh_uv = scale * mesh_xyz[..., :2] + t (utils/utils.py:47-63,
                                       models/dir.py:278-280,359-361); read only where mesh_uv is NULL */
    const float* joint_xyz[2];      /* pd_joint_xyz_* [B,21,3] metres */
    const float* mesh_xyz[2];       /* pd_mesh_xyz_*  [B,778,3] metres */
    const float* offset;            /* pd_offset      [B,3] */
} dir_loss_pred;
typedef struct dir_loss_target {    /* target / meta_info of models/dir.py:543-554 */
    const float* joint_2d[2];       /* joint_2d_* [B,21,c2]: the first two columns are used (:572) */
    const float* mesh_2d[2];        /* mesh_2d_*  [B,778,c2] */
    const float* joint_3d[2];       /* joint_3d_* [B,21,3] metres */
    const float* mesh_3d[2];        /* mesh_3d_*  [B,778,3] metres */
    const float* center[2];         /* center_*   [B,3] */
    const int32_t* faces[2];        /* ManoLayer.th_faces [n_faces,3] */
    int32_t c2, n_faces;
} dir_loss_target;
/* The 13 terms of one stage (models/dir.py:571-592) in this order: joint_left_uv, joint_right_uv, mesh_left_uv, mesh_right_uv,
 * joint_left_xyz, joint_right_xyz, mesh_left_xyz, mesh_right_xyz, edge_left, edge_right, normal_left (x0.1), normal_right (x0.1),
 * offset; SmoothL1 terms x coord_weight (the reference's 10).  scratch: B*13 doubles (device); out13: 13 floats (device). */
int dir_stage_losses_forward(const dir_loss_pred* pred_host, const dir_loss_target* gt_host, float coord_weight, double* scratch,
                             float* out13, int B, void* stream);
/* models/dir.py:562-569: seg (weighted cross entropy x0.1), dense (SmoothL1), lovasz (x0.1), each x dense_weight -> out3.
 * seg_logits / dense_pred [B,3,S,S]; gt_seg [B,1,H,W] labels 0..2 stored as floats (F.interpolate nearest -> .long());
 * gt_dense [B,3,H,W] (F.interpolate bilinear).  class_weight_host: 3 floats (0.1, 0.45, 0.45).  workspace: device bytes,
 * dir_dense_losses_workspace_bytes(B, S) of them (sort keys / values, both halves of the radix sort's ping-pong, and its digit histograms). */
long long dir_dense_losses_workspace_bytes(int B, int S);
int dir_dense_losses_forward(const float* seg_logits, const float* dense_pred, const float* gt_seg, const float* gt_dense,
                             const float* class_weight_host, float dense_weight, void* workspace, long long workspace_bytes,
                             float* out3, int B, int S, int H, int W, void* stream);

/* 8f rank 2, optimiser: train.py:227 `optim.AdamW(params, lr)` (torch defaults betas (0.9, 0.999), eps 1e-8, weight_decay 0.01) as one
 * launch over flat fp32 buffers of n elements (16-byte aligned): decoupled weight decay, bias-corrected moments, torch's fp32
 * operation order.  step = 1-based update count (the value torch keeps in state['step'] AFTER this update). */
int dir_adamw_step(float* param, const float* grad, float* exp_avg, float* exp_avg_sq, long long n, double lr, double beta1,
                   double beta2, double eps, double weight_decay, long long step, void* stream);

/* Guarded AdamW step (ABI 50): gradient clipping by the global norm, skipping of a step whose gradient is not finite, and an exponential
 * moving average of the parameters, decided on the device -- the host reads nothing in order to go on.  The reference has none of the
 * three: the rule below is this project's own (clip_grad_norm_'s coefficient, GradScaler's way of skipping, timm ModelEmaV2's average),
 * restated in numpy by tests/helpers/guarded_step_ref.py.  Per step: ONE dir_grad_guard over the whole gradient (two small launches), then
 * one dir_adamw_guarded_step per parameter range (one streaming launch each), all on the same stream.
 *
 * dir_grad_guard(grad[n], ...):
 *   sumsq     = sum_i (double)g_i * (double)g_i.  Stage one: a fixed grid (a function of n only) of 256-thread workgroups, each thread
 *               accumulating its grid-stride share in double, each workgroup summing its 256 values in a fixed tree and writing ONE
 *               double to workspace[workgroup index]; stage two: one workgroup sums those in index order and the same tree.  No
 *               floating-point atomics, no completion counters: the same n and bytes give the same bits on every run.  A gradient of
 *               1e30 squares to 1e60 in double (finite).  workspace: dir_grad_norm_workspace_bytes(n) bytes (device, 8-byte aligned;
 *               a pure host function, -1 for n <= 0).
 *   norm      = sqrt(sumsq);  nonfinite = !isfinite(sumsq)  (one NaN or Inf anywhere in grad[0..n) sets it)
 *   coef      = (float)min(1.0, max_norm / (norm + 1e-6))   (max_norm = +inf: 1.0f; min(1.0, NaN) = 1.0)
 *   skip      = skip_nonfinite && nonfinite
 *   skip:       skipped += 1, skipped_in_row += 1; bc1, bc2_sqrt keep their values
 *   otherwise:  applied += 1, skipped_in_row = 0, clipped += (coef < 1);
 *               bc1 = 1 - beta1^applied (double), bc2_sqrt = (float)sqrt(1 - beta2^applied): dir_adamw_step's prefactors for
 *               step = applied.  A skipped step does not advance AdamW's step count.
 *   The counters are read-modify-written: the caller zeroes the state once (or writes the counts to continue from) and never again.
 *
 * dir_adamw_guarded_step(...): dir_adamw_step's arithmetic, operation for operation, with
 *   g'        = g * coef                       (one float multiply, not contracted: the bits g.mul_(coef) leaves)
 *   step_size = (float)(lr / state->bc1), bc2_sqrt = state->bc2_sqrt;  lr, betas, eps, weight_decay are host arguments as before
 *   ema       (may be NULL) after the parameter update, with w = (float)(1 - ema_decay), not contracted, torch's lerp_(p, w):
 *               e = e + w * (p_new - e)            for w <  0.5  (every decay in use)
 *               e = p_new - (p_new - e) * (1 - w)  for w >= 0.5  (decay = 0 returns p_new itself)
 *   state->skip set: the kernel returns before any load or store: param, exp_avg, exp_avg_sq and ema keep their bits.
 * Both check their arguments (null pointers, alignment, n <= 0, max_norm <= 0 or NaN, ema_decay outside [0, 1], workspace too small)
 * before anything is launched. */
typedef struct dir_guard_state {
    double sumsq, norm;                 /* of the last dir_grad_guard */
    double bc1;                         /* 1 - beta1^applied */
    long long applied, skipped, skipped_in_row, clipped;
    float coef;                         /* of the last dir_grad_guard */
    float bc2_sqrt;                     /* sqrt(1 - beta2^applied) */
    int32_t nonfinite, skip;            /* of the last dir_grad_guard */
    int32_t reserved[2];
} dir_guard_state;     /* 80 bytes */
long long dir_grad_norm_workspace_bytes(long long n);
int dir_grad_guard(const float* grad, long long n, double max_norm, int skip_nonfinite, double beta1, double beta2, void* workspace,
                   long long workspace_bytes, dir_guard_state* state, void* stream);
int dir_adamw_guarded_step(float* param, const float* grad, float* exp_avg, float* exp_avg_sq, float* ema, long long n, double lr,
                           double beta1, double beta2, double eps, double weight_decay, double ema_decay, const dir_guard_state* state,
                           void* stream);

/* a13 backward, first step of the training backward pass (8f rank 2): gradients of (sum_k grad_out[k] * term_k) w.r.t. the predictions
 * the terms read -- what autograd gives through models/loss.py / models/lovasz_loss.py / nn.CrossEntropyLoss as models/dir.py:562-592
 * composes them.  grad_out: device pointer to the upstream gradients of the 13 (3) terms in forward order, or NULL for ones.
 * pd_mesh_uv is an independent input here (pred->mesh_uv must be given; the projection's chain rule is the caller's).
 * vert_face_offsets[h] [779] / vert_face_index[h] [3 n_faces]: CSR lists vertex -> (face * 3 + corner) of faces[h] (int32, device):
 * vertex gradients are summed in that order, without atomics (deterministic). */
typedef struct dir_loss_pred_grad {
    float* joint_uv[2]; float* mesh_uv[2]; float* joint_xyz[2]; float* mesh_xyz[2]; float* offset;     /* same shapes as dir_loss_pred */
} dir_loss_pred_grad;
int dir_stage_losses_backward(const dir_loss_pred* pred_host, const dir_loss_target* gt_host, float coord_weight, const float* grad_out13,
                              const int32_t* const* vert_face_offsets, const int32_t* const* vert_face_index,
                              const dir_loss_pred_grad* grads_host, int B, void* stream);
long long dir_dense_losses_backward_workspace_bytes(int B, int S);
/* grad_seg / grad_dense: [B,3,S,S] fp32 */
int dir_dense_losses_backward(const float* seg_logits, const float* dense_pred, const float* gt_seg, const float* gt_dense,
                              const float* class_weight_host, float dense_weight, const float* grad_out3, void* workspace,
                              long long workspace_bytes, float* grad_seg, float* grad_dense, int B, int S, int H, int W, void* stream);

/* ---------------------------------------------------------------------------------------------------------------------------------
 * f3, from files: the GPU half of the JPEG decode (round 5).  cv.imread of the reference's input pipeline (apps/eval.py:56,
 * dataset/interhand.py:223 over dataset/prepare_data.py:123-166's files) = libjpeg's default decode.  The host decodes the Huffman stream only
 * (include/dir_jpeg.h: dir_jpeg_decode_coefficients -> one record per image = dir_jpeg_header + quantised int16 coefficients); this entry point
 * takes a batch of records that sit `record_stride` bytes apart in device memory and writes the uint8 BGR frames [B,H,W,3] that
 * dir_stem_pool_forward(_dt) / dir_stem_prep_s2d_u8 / dir_image_normalize_forward read: dequantisation, the "islow" integer IDCT with its range
 * limit, "fancy" h2v2 / h2v1 chroma upsampling, 16-bit fixed-point YCbCr -> RGB -- integer arithmetic, bit-exact with libjpeg(-turbo)
 * (oracle/jpeg.py, pinned to Pillow's decoder).  Every record must describe an H x W image (4:2:0, 4:2:2, 4:4:4 or grayscale); a record that
 * does not sets *err_flag (device int32, zeroed by the caller) to 1 + its index and its frame is left untouched.
 * planes_scratch: B x round_up_16(dir_jpeg_planes_bytes(record_stride)) bytes of device memory. */
long long dir_jpeg_planes_bytes(long long record_bytes);
int dir_jpeg_decode_records(const void* records, long long record_stride, int B, int H, int W, void* planes_scratch, long long scratch_bytes, void* out_bgr,
                            int32_t* err_flag, void* stream);

/* ---------------------------------------------------------------------------------------------------------------------------------
 * To files: the GPU half of the JPEG ENCODE (ABI 51), the mirror image of dir_jpeg_decode_records.  cv.imwrite of the reference's
 * dataset/prepare_data.py:174-214 (mask/ and dense/ frames) = libjpeg's default compression.  This entry point does everything before the
 * Huffman coder, in one launch: uint8 frames [B,H,W,3] (HWC; channel_order 0 = B,G,R -- what cv.imwrite receives, the project's frame
 * convention -- or 1 = R,G,B) -> B coefficient records `record_stride` bytes apart, each a dir_jpeg_header + int16 coefficients
 * [component][block row][block column][64] in natural order: byte for byte what dir_jpeg_decode_coefficients (include/dir_jpeg.h) writes
 * when it reads the file libjpeg(-turbo) writes for the frame.  The host turns a record into that file (include/dir_jpeg_enc.h:
 * dir_jpeg_encode_record).  Bytes of a slot beyond the record (dir_jpeg_record_bytes(W, H, 2, 2, 3)) are not touched.
 *
 * Scope: three components, 4:2:0, 8-bit samples, H and W multiples of 16 (whole MCUs: no edge replication, no dummy blocks), each at most
 * 4096, table entries 1..255.  Anything else returns DIR_E_INVALID before any launch (callers keep their host encoder for such frames).
 *
 * The rule (libjpeg's, integer and exact; int32 suffices for 8-bit samples):
 *   tables     luma_q / chroma_q: HOST pointers to uint16[64] in natural order, e.g. dir_jpeg_quality_tables (jpeg_set_quality(q, TRUE):
 *              s = 5000 / q for q < 50, else 200 - 2 q; entry = clamp((base * s + 50) / 100, 1, 255) over the Annex K tables); passed to
 *              the kernel by value and copied into every header (quant[0] = luma, quant[1] = quant[2] = chroma)
 *   colour     jccolor.c, FIX(x) = int(x * 65536 + 0.5):
 *                Y  = ( FIX(.299) R + FIX(.587) G + FIX(.114) B + 32768) >> 16
 *                Cb = (-FIX(.16874) R - FIX(.33126) G + FIX(.5) B + (128 << 16) + 32767) >> 16
 *                Cr = ( FIX(.5) R - FIX(.41869) G - FIX(.08131) B + (128 << 16) + 32767) >> 16
 *   chroma     jcsample.c h2v2_downsample without smoothing: (a + b + c + d + bias) >> 2 over each 2 x 2 group, bias 1 for even output
 *              columns and 2 for odd ones
 *   DCT        jfdctint.c ("islow") on sample - 128, CONST_BITS 13, PASS1_BITS 2: rows first (results scaled up by 4), then columns
 *              (DESCALE by PASS1_BITS for outputs 0 and 4, by CONST_BITS + PASS1_BITS for the others), its twelve constants,
 *              DESCALE(x, n) = (x + (1 << (n - 1))) >> n; the results carry libjpeg's factor 8
 *   quantise   sign(c) * ((|c| + (8 q >> 1)) / (8 q))   (jcdctmgr.c; computed with an exact reciprocal: the same integers)
 *   header     magic DIR_JPEG_MAGIC, width, height, ncomp 3, hmax = vmax = 2, mcux = W / 16, mcuy = H / 16, h = v = {2, 1, 1},
 *              blocks_x = {2 mcux, mcux, mcux}, blocks_y likewise, coef_offset = {0, 256 n, 320 n} and total_coef = 384 n for n = mcux mcuy,
 *              the tables, reserved words zero
 * An MCU depends on nothing but its own 16 x 16 pixels: no atomics, no scratch, no workspace, no host read; capturable in a graph; an
 * image gives the same bytes in any slot of any batch.  frames: 4-byte aligned; records: 16-byte aligned, record_stride a multiple of 16. */
int dir_jpeg_encode_records(const void* frames, int B, int H, int W, int channel_order, const uint16_t* luma_q, const uint16_t* chroma_q,
                            void* records, long long record_stride, void* stream);


/* ---- training input: dataset/interhand.py:__getitem__ of split 'train' (utils/utils.py:202-207, 406-533) for a batch (csrc/augment.hip) ----
 * Frames are uint8 BGR HWC [B,256,256,3] as dir_jpeg_decode_records writes them; 256 = the reference's img_size.  One dir_aug_params per image,
 * in DEVICE memory (the host sampler of dir_amd/apps/trainset.py fills them):
 *   M       get_affine_mat's float32 2x3 matrix (output pixel = M * source pixel of the flipped frame); inverted in double as cv.warpAffine does
 *   flip    1: the frames are mirrored (img[:, ::-1]) before blur and warp; seg labels 1 / 2 swap; the labels swap left / right and x -> 255 - x
 *   blur    motion-blur kernel size 1..DIR_AUG_MAX_BLUR (the reference draws 3..9); any other value: no blur
 *   a, b    add_noise's per-channel gain (channel order B, G, R) and offset, fp64
 *   kernel  the blur x blur float32 motion-blur kernel, row-major */
#define DIR_AUG_MAX_BLUR 9
#define DIR_AUG_MAX_BATCH 4096
typedef struct dir_aug_params {
    float M[6];
    int32_t flip;
    int32_t blur;
    double a[3];
    double b;
    float kernel[DIR_AUG_MAX_BLUR * DIR_AUG_MAX_BLUR];
    float pad_[3];
} dir_aug_params;   /* 400 bytes */
/* The Gaussian term 255 * N(0, 0.01) of add_noise, float32 [B,256,256,3], element (image b, pixel p = y * 256 + x, channel c):
 *   h  = splitmix64(splitmix64(seed) + (b * 65536 + p) * 3 + c)        (splitmix64: z += 0x9E3779B97F4A7C15, then the usual two
 *                                                                        xor-shift-multiply rounds 30 / 0xBF58476D1CE4E5B9, 27 / 0x94D049BB133111EB, 31)
 *   u1 = ((h >> 41) + 0.5) * 2^-23,  u2 = (h & 0xFFFFFF) * 2^-24
 *   n  = 2.55f * sqrtf(-2 logf(u1)) * cosf(2 pi u2)                    (Box-Muller, float32)
 * Deterministic per (seed, b, p, c); dir_train_augment_images with noise = NULL generates exactly this field in-line. */
int dir_train_noise_field(unsigned long long seed, float* out, int B, void* stream);
/* The image side, two launches.  (1) filter2D (reflect-101 border, anchor blur / 2) of every img whose params ask for blur, from the flipped
 * frame into blur_scratch (uint8 [B,256,256,3], caller-owned; rows of other images are not touched): per channel s = 0.f, then
 * s = s + k[r][q] * src for r, q in row-major order (float32, no fused multiply-add), rounded half to even and clamped (saturate_cast<uchar>).
 * (2) per output pixel: cv.warpAffine INTER_LINEAR of img (blurred or not) / mask / dense -- inverse in double, coordinates in 10-bit fixed
 * point rounded to 5 bits, 15-bit weights summing to 32768, a tap outside the frame reads 0, (sum + 2^14) >> 15 --; seg from the warped mask
 * (hand = G > 50 | R > 50, left = G >= R -> 1, right -> 2, swapped when flipped); add_noise in fp64 (a * v + b + noise, clip 0..255,
 * truncated to uint8) with `noise` (float32 [B,256,256,3], or NULL: dir_train_noise_field(seed)).  Outputs (fp32):
 *   img_nchw [B,3,256,256]  RGB / 255, (t - mean) / std of the noised frame (== dir_image_normalize_forward, bit for bit; mean / std host)
 *   img_rgb  [B,256,256,3]  the noised uint8 BGR frame as float (NULL to skip)      mask_rgb [B,256,256,3] the warped mask (NULL to skip)
 *   seg      [B,1,256,256]                                                          dense_out [B,3,256,256] the warped dense frame / 255 */
int dir_train_augment_images(const dir_aug_params* params, const uint8_t* img, const uint8_t* mask, const uint8_t* dense,
                             const float* noise, unsigned long long seed, const float* mean_host, const float* std_host,
                             uint8_t* blur_scratch, float* img_nchw, float* img_rgb, float* mask_rgb, float* seg,
                             float* dense_out, int B, void* stream);
/* The label side, one launch, fp64 inside, one rounding to fp32 per output.  in_host: 8 device pointers, the gt_batch outputs
 * joint_xyz L [B,21,3], mesh_xyz L [B,778,3], joint_xyz R, mesh_xyz R (camera space), joint_uv L [B,21,2], mesh_uv L [B,778,2], joint_uv R, mesh_uv R;
 * camera [B,3,3].  out_host: 10 device pointers, joint_2d L [B,21,3], mesh_2d L [B,778,3], joint_2d R, mesh_2d R, joint_3d L [B,21,3],
 * mesh_3d L [B,778,3], joint_3d R, mesh_3d R, center L [B,1,3], center R [B,1,3].  With params: the flip (x -> 256 - x - 1, left <-> right),
 * uv' = M uv, xyz = uvd2xyz_np(uv', z); without (NULL, the val / test splits): xyz and uv as they are.  2D targets = (uv / 256 * 2 - 1, z);
 * center = joint 9 of the 3D target. */
int dir_train_augment_labels(const dir_aug_params* params, const float* const* in_host, const float* camera, float* const* out_host,
                             int B, void* stream);

/* ---- two-hand mesh rasteriser: dataset/prepare_data.py:174-214 (render_data) through mano_two_hands_renderer (csrc/render.hip) ----
 * The rules (pytorch3d's rasterize_meshes with blur_radius 0, faces_per_pixel 1, perspective-correct barycentrics, no culling, no z
 * clipping; HardPhongShader + AmbientLights) are written out in the header comment of csrc/render.hip.  Device pointers:
 *   verts   float32 [B,1556,3] camera frame, left hand 0..777, right 778..1555
 *   faces   int32 [3076,3]: left = right faces with columns [1,0,2], right = right faces + 778 (an index outside 0..1555 skips the face)
 *   K       float32 [B,3,3] intrinsics of the S x S image
 *   colors  float32 [1556,3] per-vertex colour table (0..255 scale), needed by color_u8 / color_f32 only
 * Outputs, each written when its pointer is not NULL (at least one):
 *   pix_to_face  int32 [B,S,S]      face index within the mesh (0..3075), -1 background
 *   zbuf         float32 [B,S,S]    view-space depth of the face, -1 background
 *   bary         float32 [B,S,S,3]  perspective-correct barycentrics, -1 background
 *   mask         uint8 [B,S,S,3]    the mask frame cv.imwrite receives (left (0,0,255), right (0,255,0), background 1)
 *   color_u8     uint8 [B,S,S,3]    the frame of `colors` cv.imwrite receives (background 1)
 *   color_f32    float32 [B,S,S,3]  texel / 255 of `colors` (the renderer's image; background 1/255)
 * workspace: dir_render_workspace_bytes(B) bytes of device memory (per-face tile ranges).  S in 16..1024. */
#define DIR_RENDER_VERTS 1556
#define DIR_RENDER_FACES 3076
#define DIR_RENDER_MIN_SIZE 16
#define DIR_RENDER_MAX_SIZE 1024
#define DIR_RENDER_MAX_BATCH 4096
long long dir_render_workspace_bytes(int B);
int dir_render_two_hands(const float* verts, const int32_t* faces, const float* K, const float* colors, int B, int S, void* workspace,
                         long long workspace_bytes, int32_t* pix_to_face, float* zbuf, float* bary, uint8_t* mask, uint8_t* color_u8,
                         float* color_f32, void* stream);

/* ---- shaded and orthographic rendering of the same two-hand mesh: mano_two_hands_renderer.render_rgb / render_rgb_orth and the
 * scale= / trans2d= cameras (utils/vis_utils.py:138-149, 278-330; HardPhongShader with PointLights, default Materials / BlendParams).
 * The rules are written out in the header comment of csrc/render.hip.  Device pointers unless said otherwise:
 *   adjacency  dir_render_adjacency_bytes() bytes, made once per face table by dir_render_adjacency: for every vertex its incident
 *              (face, corner) pairs in ascending face index, so that the vertex normals are summed in a fixed order
 *   normals    float32 [B,1556,3] vertex normals in world space (pytorch3d's verts_normals_packed)
 *   K          float32 [B,3,3], the perspective camera; OR
 *   scale      float32 [B] and trans2d float32 [B,2], the orthographic camera (focal 2 scale, principal point -trans2d,
 *              R = diag(-1,-1,1), T = (0,0,10)).  Exactly one camera kind is given; the other kind's pointers are NULL.
 *   colors     float32 [1556,3] vertex colours (0..255), lights: HOST pointer; both needed by shaded_f32 / overlay_u8, as is adjacency
 *   background uint8 [B,S,S,3] or NULL: the frame that shows through where no face covers the pixel (overlay_u8 only)
 * Outputs, each written when its pointer is not NULL (at least one): pix_to_face / zbuf / bary as dir_render_two_hands (under the
 * orthographic camera zbuf is z + 10 and bary are the plain screen-space barycentrics),
 *   shaded_f32  float32 [B,S,S,3]  colour / 255, background 1/255
 *   overlay_u8  uint8 [B,S,S,3]    round_half_even(clamp(fl32(colour / 255) * 255, 0, 255)) where a face covers the pixel, else the
 *                                  background frame's bytes (1 without a frame)
 * workspace: dir_render_shaded_workspace_bytes(B) bytes (tile ranges + vertex normals).  shininess must be 64. */
typedef struct dir_render_lights {
    float ambient[3], diffuse[3], specular[3];      /* light colour x material colour per channel (the default Materials are 1) */
    float location[3];                              /* the point light, world space */
    float shininess;                                /* 64: the power is taken as six successive squarings */
} dir_render_lights;
long long dir_render_adjacency_bytes(void);
int dir_render_adjacency(const int32_t* faces, void* adjacency, long long adjacency_bytes, void* stream);
int dir_render_vertex_normals(const float* verts, const int32_t* faces, const void* adjacency, int B, float* normals, void* stream);
long long dir_render_shaded_workspace_bytes(int B);
int dir_render_shaded(const float* verts, const int32_t* faces, const void* adjacency, const float* K, const float* scale,
                      const float* trans2d, const float* colors, const dir_render_lights* lights, const uint8_t* background, int B, int S,
                      void* workspace, long long workspace_bytes, int32_t* pix_to_face, float* zbuf, float* bary, float* shaded_f32,
                      uint8_t* overlay_u8, void* stream);

/* Predicted 2-D joints drawn over a picture, in place: image uint8 [B,S,S,3], uv_left / uv_right float32 [B,21,2] in -1..1 (pd_joint_uv_*;
 * joint 0 the wrist, then four joints per finger, thumb first).  Discs of joint_radius pixels and bones of half-width bone_radius, by this
 * project's own coverage rule and palette (csrc/render.hip) -- it is NOT OpenCV's drawing. */
int dir_render_joints(uint8_t* image, const float* uv_left, const float* uv_right, int B, int S, float joint_radius, float bone_radius,
                      void* stream);

/* ---- inter-hand penetration: how far two meshes pass through each other (csrc/penetration.hip) ----
 * The measures are ObMan's (Hasson et al. 2019); the rules (generalised winding number with |w| > 0.5 as the inside test, closest point
 * on the closed triangle, which faces are skipped, the voxel lattice) are written out in the header comment of csrc/penetration.hip.
 * Generic in the mesh sizes.  Device pointers:
 *   verts_a  float32 [B,Va,3], faces_a int32 [Fa,3]; verts_b float32 [B,Vb,3], faces_b int32 [Fb,3]: two batched meshes in ONE frame,
 *            each with one face table for the whole batch.  A face with a repeated index or an index outside 0..V-1 is skipped.
 * dir_mesh_penetration queries A's vertices against mesh B (direction 0) and B's against A (direction 1):
 *   winding, dist  float32 [B,Va+Vb] or NULL: per vertex, A's vertices first, the winding number with respect to the OTHER mesh and the
 *                  distance to its surface (metres; +inf when every face is skipped)
 *   count          int32 [B,2]    vertices inside the other mesh, per direction
 *   max_depth      float32 [B,2]  the largest distance over those vertices, 0 when there are none
 *   sum_depth      float32 [B,2]  the sum of the distances over those vertices
 * The results are the same bits from run to run and for a sample in any batch.
 * dir_mesh_intersection_volume counts the points of the lattice (i h, j h, k h) inside both meshes, over the intersection of the two
 * bounding boxes; everything is decided on the device:
 *   cells    int32 [B]    lattice points in the boxes' intersection (0: the boxes are disjoint); max_cells + 1 when there are more than
 *                         max_cells, or when a lattice index exceeds 2^24 -- then nothing is examined
 *   n_both   int32 [B]    lattice points inside both meshes (0 when nothing was examined)
 *   volume   float32 [B]  n_both * h^3 (cubic metres), NaN when nothing was examined because of max_cells
 * Sizes outside the limits below, B <= 0, h <= 0 or a null pointer give DIR_E_INVALID before any launch. */
#define DIR_MESH_MAX_VERTS 4096
#define DIR_MESH_MAX_FACES 8192
#define DIR_MESH_MAX_BATCH 65536
#define DIR_MESH_MAX_CELLS (1 << 24)
int dir_mesh_penetration(const float* verts_a, const int32_t* faces_a, const float* verts_b, const int32_t* faces_b, int B, int Va, int Fa,
                         int Vb, int Fb, float* winding, float* dist, int32_t* count, float* max_depth, float* sum_depth, void* stream);
int dir_mesh_intersection_volume(const float* verts_a, const int32_t* faces_a, const float* verts_b, const int32_t* faces_b, int B, int Va,
                                 int Fa, int Vb, int Fb, float h, int max_cells, float* volume, int32_t* n_both, int32_t* cells,
                                 void* stream);

/* ---- aligned evaluation measures: Procrustes-aligned errors, nearest-neighbour distances, threshold counts (csrc/alignmetric.hip) ----
 * Generic in the point count.  Device pointers, float32 arithmetic, no floating-point atomics; every output of a sample is the same
 * bits from run to run and in any batch.
 * dir_procrustes_align fits, per sample, the similarity that maps pd onto gt in the least-squares sense (Umeyama 1991), with
 * p = pd - mean(pd), g = gt - mean(gt): R the PROPER rotation (det +1, never a reflection) that maximises sum g_i . R p_i, found as Horn's
 * unit quaternion by Jacobi sweeps; s = sum g_i . R p_i / sum |p_i|^2 with DIR_ALIGN_SCALE in flags, 1 without; t = mean(gt) - s R mean(pd).
 *   pd, gt     float32 [B,N,3], 3 <= N <= DIR_MESH_MAX_VERTS
 *   transform  float32 [B,13] or NULL: s, R row-major, t
 *   aligned    float32 [B,N,3] or NULL: s R pd + t
 *   err        float32 [B,N]: |aligned - gt|
 * A sample with a non-finite coordinate or with sum |p_i|^2 = 0 gets NaN in all of its outputs.  Where the maximiser is not unique
 * (collinear points) one of them is returned: finite, and a proper rotation.
 * dir_point_set_nn: a float32 [B,Na,3], b float32 [B,Nb,3], 1 <= Na, Nb <= DIR_MESH_MAX_VERTS;
 *   d_ab  float32 [B,Na]: the distance from each point of a to its nearest point of b (point to point); d_ba float32 [B,Nb]: the reverse.
 * Non-finite points of the searched set are passed over (+inf when none is left); a non-finite query point gives NaN.
 * dir_threshold_counts ADDS to counts (int64 [K+1]): counts[k] gains the number of finite err[i] <= thresholds[k], counts[K] the
 * number of finite values examined.  err float32 [n], 1 <= n <= DIR_ALIGN_MAX_VALUES; thresholds float32 [K], 1 <= K <=
 * DIR_ALIGN_MAX_THRESHOLDS, in any order.
 * A null required pointer, B <= 0 or a size outside these limits gives DIR_E_INVALID before any launch. */
#define DIR_ALIGN_SCALE 1
#define DIR_ALIGN_MAX_THRESHOLDS 1024
#define DIR_ALIGN_MAX_VALUES 2147483647LL
int dir_procrustes_align(const float* pd, const float* gt, int B, int N, int flags, float* transform, float* aligned, float* err,
                         void* stream);
int dir_point_set_nn(const float* a, const float* b, int B, int Na, int Nb, float* d_ab, float* d_ba, void* stream);
int dir_threshold_counts(const float* err, long long n, const float* thresholds, int K, long long* counts, void* stream);

/* ---- hand crops from full frames: dataset/dataset_utils.py:26-58 (cut_img) for frames of any size (csrc/crop.hip) ----
 * The crop matrix rule is cut_img's in float64 (inputs converted to double first; every operation rounded on its own).  From the
 * per-axis Min / Max of a point set, or of the two corners of a tight box (frame pixel positions, OpenCV's convention):
 *   mid = (Min + Max) / 2,  L = max(Max - Min) / 2 / ratio,  s = (size / 2) / L,  M = [[s, 0, s (L - mid_x)], [0, s, s (L - mid_y)]]
 * valid = 0, and the matrix is written as zeros, when an input is not finite, L is not finite and positive, s lies outside
 * [DIR_CROP_MIN_SCALE, DIR_CROP_MAX_SCALE], or one of mid_x - L, mid_x + L, mid_y - L, mid_y + L (the source coordinates of the crop's
 * corners) exceeds DIR_CROP_MAX_COORD in magnitude -- that bound keeps the 10-bit fixed-point source coordinates inside an int32.
 * All three entry points allocate nothing and read nothing back.  Device pointers; M is double [B,6] row-major, valid int32 [B].
 *
 * dir_crop_matrices_from_boxes: boxes float32 [B,4] = (x0, y0, x1, y1), the tight box around both hands.
 * dir_crop_matrices_from_meshes, the tracking step: the box of frame t + 1 from the prediction of frame t.  mesh_left / mesh_right float32
 * [B,778,3], proj_left / proj_right float32 [B,3] = (s, tx, ty) of one stage of DIR.forward, M_prev the matrix frame t was cropped with.
 * Per vertex: uv = s xy + t in float32 (multiply, then add: utils/utils.py:47-63); crop position c = (uv + 1) size / 2 in double (the
 * inverse of dataset/interhand.py:229-232); frame position p = (c - (M_prev[2], M_prev[5])) / M_prev[0].  Min / Max over the 1 556
 * positions go through the rule above.  Minimum and maximum do not depend on the order, so a sample gives the same bits in any batch.
 * Where the result is invalid (a non-finite position included) M_next = M_prev and valid = 0: the box holds.  M_next may be M_prev.
 *
 * dir_crop_frames: out uint8 [B,size,size,3] = cv.warpAffine(frame_b, M_b, (size, size)), INTER_LINEAR, BORDER_CONSTANT 0, for a ragged
 * batch: `frames` is one packed buffer of frames_bytes bytes holding uint8 BGR images, descs [B] says where each one lies.  M is any
 * invertible 2x3 matrix, inverted in double as cv.warpAffine does; the fixed-point rules are dir_train_augment_images'.  status int32 [B]
 * (or NULL) receives, per image, 0 or the reason its crop is all zeros:
 *   DIR_CROP_INVALID     valid[b] == 0 (valid may be NULL: every matrix is used)
 *   DIR_CROP_BAD_DESC    height or width outside 1..DIR_CROP_MAX_SIDE, row_stride < 3 width or > DIR_CROP_MAX_STRIDE, offset < 0, or
 *                        offset + (height - 1) row_stride + 3 width > frames_bytes
 *   DIR_CROP_BAD_MATRIX  a non-finite entry of the inverse m, or |m0| (size - 1) + |m1| (size - 1) + |m2| > DIR_CROP_MAX_COORD (likewise m3, m4,
 *                        m5): a source coordinate that far out, whose fixed-point terms could leave an int32
 * No byte outside [frames, frames + frames_bytes) is read.  size in DIR_CROP_MIN_SIZE..DIR_CROP_MAX_SIZE, B in 1..DIR_CROP_MAX_BATCH
 * (B = 0 is a no-op); out needs 4-byte alignment.
 *
 * dir_crop_frames_area: dir_crop_frames with anti-aliasing where the crop shrinks the frame.  Arguments, statuses and the black crop of a
 * refused image are dir_crop_frames'; `area` int32 [B] (or NULL) receives 1 for the images that got the rule below, else 0.  Two launches,
 * no host read, no workspace: the matrices may come straight from dir_crop_matrices_from_meshes.  An image gets the same bytes in any
 * batch and at any position of it.
 *   Which images: M is "shrinking" when M[1] == 0 and M[3] == 0, M[0] > 0 and M[4] > 0, and min(M[0], M[4]) < 1.  Every other usable
 *   matrix (a scale >= 1, a rotation, a shear, a mirror) gives exactly dir_crop_frames' bytes.  A shrinking matrix that dir_crop_frames
 *   would refuse, or whose min(M[0], M[4]) < DIR_CROP_MIN_SCALE, is DIR_CROP_BAD_MATRIX: that bound keeps a window at 2 * 64 + 1 taps.
 *   The rule is Pillow's Image.resize((size, size), BILINEAR, box) -- libImaging/Resample.c: precompute_coeffs and normalize_coeffs_8bpc with
 *   PRECISION_BITS = 22, horizontal pass, then vertical pass -- on the box the matrix cuts out of the frame, without Pillow's clamping of
 *   the window to the image.  Per axis (x shown; s = M[0], t = M[2]; y: M[4], M[5]), in float64, every operation rounded on its own:
 *     in0 = 0.5 - (t + 0.5) / s,  in1 = in0 + size / s          the crop's edges in frame pixels (pixel k covers [k, k + 1))
 *     scale = (in1 - in0) / size,  fs = max(scale, 1),  support = fs
 *   and per output position u:
 *     c = in0 + (u + 0.5) scale,  xmin = floor(c - support + 0.5),  xmax = floor(c + support + 0.5),  taps x = xmin .. xmax - 1
 *     k[x] = max(0, 1 - |(x - c + 0.5) / fs|),  ww = the sum of k in tap order,  K[x] = (int)(k[x] / ww * 2^22 + 0.5)
 *   A tap outside the frame reads 0 and keeps its weight (the zero border of dir_crop_frames; Pillow on a frame padded with zeros); it is
 *   never loaded.  Horizontal pass: tmp = clip8((2^21 + sum K_x src) >> 22), stored as uint8 -- the rounding between the passes is part of
 *   the rule; vertical pass: the same over tmp with the rows' coefficients.  The integer sums are exact in any order. */
#define DIR_CROP_MIN_SCALE 0.015625 /* 2^-6 */
#define DIR_CROP_MAX_SCALE 64.0
#define DIR_CROP_MAX_COORD 1048576.0 /* 2^20 */
#define DIR_CROP_MIN_SIZE 16
#define DIR_CROP_MAX_SIZE 1024
#define DIR_CROP_MAX_BATCH 4096
#define DIR_CROP_MAX_SIDE 65536
#define DIR_CROP_MAX_STRIDE 1048576
#define DIR_CROP_INVALID 1
#define DIR_CROP_BAD_DESC 2
#define DIR_CROP_BAD_MATRIX 3
typedef struct dir_frame_desc {
    long long offset;       /* of the image's first byte in the packed buffer */
    int32_t height, width;
    long long row_stride;   /* bytes from one row to the next, >= 3 width */
} dir_frame_desc;           /* 24 bytes */
int dir_crop_matrices_from_boxes(const float* boxes, int B, double ratio, int size, double* M, int32_t* valid, void* stream);
int dir_crop_matrices_from_meshes(const float* mesh_left, const float* mesh_right, const float* proj_left, const float* proj_right,
                                  const double* M_prev, int B, double ratio, int size, double* M_next, int32_t* valid, void* stream);
int dir_crop_frames(const uint8_t* frames, long long frames_bytes, const dir_frame_desc* descs, const double* M, const int32_t* valid,
                    int B, int size, uint8_t* out, int32_t* status, void* stream);
int dir_crop_frames_area(const uint8_t* frames, long long frames_bytes, const dir_frame_desc* descs, const double* M, const int32_t* valid,
                         int B, int size, uint8_t* out, int32_t* status, int32_t* area, void* stream);

/* ---- temporal smoothing of tracked predictions: the One-Euro filter with a jitter measure (csrc/smooth.hip) ----
 * Casiez, Roussel, Vogel, "1 Euro Filter", CHI 2012: an exponential filter whose cutoff rises with the filtered speed.  The reference has
 * no temporal code: the rule below is this project's own, restated in float64 numpy by tests/helpers/one_euro_ref.py.  One launch per
 * frame over every stream of every sequence, state updated in place, no atomics, no workspace, no host read; capturable in a graph.
 *   x        float32 [B,F]: one row per sequence, this frame's values.  A row is a list of S <= DIR_ONE_EURO_MAX_SEGMENTS segments, each
 *            n_points points of dims (1..4) components, point-major; F = sum n_points dims <= DIR_ONE_EURO_MAX_VALUES.  A POINT gets one
 *            cutoff.  `segments` is a HOST array, passed to the kernel by value.
 *   valid    int32 [B] or NULL;  y float32 [B,F], may be x;  updated int32 [B]
 *   state    B rows of dir_one_euro_state_bytes(F, S, offsets) bytes each, zeroed by the caller before the first frame, 8-byte aligned.
 *            offsets[9] (or NULL) receives the byte offsets inside a row of: jitter (double [S,2]: raw, filtered), y1, y2 (the last two
 *            outputs), x1, x2 (the last two raw inputs), dxhat (float32 [F] each), age, run, count (int32).  The state is row-major per
 *            sequence: the first B rows of a larger state are the state of a smaller batch (sequences end from the tail).  age: 0 =
 *            never initialised, else frames since the last update (saturating); run: consecutive updates.
 *            dir_one_euro_state_bytes is a pure host function; -1 for F or S outside their limits.
 * Per row:
 *   1. usable iff valid is NULL or valid[b] != 0, and all F inputs are finite.
 *   2. not usable: y = x bit for bit; age += 1 if age > 0; run = 0; updated = 0; nothing else changes.
 *   3. usable with age == 0 or age > max_gap: y = x, dxhat = 0, age = 1, run = 1, updated = 2 (initialised).
 *   4. otherwise: dt = age / fps;  alpha(fc) = 1 / (1 + 1 / (2 pi fc dt));  per component dx = (x - y1) / dt, dxhat += alpha(d_cutoff)
 *      (dx - dxhat);  per point v = speed_scale |dxhat|_2 over its components, fc = min_cutoff + beta v, y = y1 + alpha(fc) (x - y1): a
 *      constant input comes out bit for bit.  Then age = 1, run += 1, updated = 1.  Float32 arithmetic, every operation rounded on its
 *      own; dt, 2 pi dt and alpha(d_cutoff) are computed in double and rounded once.
 *   5. jitter: when run >= 3 after the update, jitter[s] gains the sum over the segment's points of |x - 2 x1 + x2|_2 (raw) and of
 *      |y - 2 y1 + y2|_2 (filtered), in double, and count gains 1.  Per-lane partials in point order, then a fixed tree: the same bits
 *      from run to run.
 *   6. x2 = x1, x1 = x, y2 = y1, y1 = y.
 * A sequence gives the same bits in any batch slot of any batch size.
 * A null pointer (valid aside), B outside 1..DIR_CROP_MAX_BATCH, S outside 1..DIR_ONE_EURO_MAX_SEGMENTS, dims outside 1..4, F over the
 * limit, fps, min_cutoff or d_cutoff <= 0, beta < 0 or max_gap < 1 gives DIR_E_INVALID before any launch. */
#define DIR_ONE_EURO_MAX_SEGMENTS 16
#define DIR_ONE_EURO_MAX_VALUES 16384
typedef struct dir_one_euro_segment {
    int32_t n_points, dims;
    float speed_scale;      /* the speed's unit: v = speed_scale |dxhat| (1000 for metres -> mm/s) */
} dir_one_euro_segment;     /* 12 bytes */
long long dir_one_euro_state_bytes(int F, int S, long long* offsets);
int dir_one_euro_step(const float* x, const int32_t* valid, int B, const dir_one_euro_segment* segments, int S, double fps, double min_cutoff,
                      double beta, double d_cutoff, int max_gap, void* state, float* y, int32_t* updated, void* stream);

/* ---- smoothing in MANO parameter space (ABI 53; csrc/para_smooth.hip; nothing in the reference) ----
 * dir_one_euro_step filters every output point alone: bone lengths are not kept, the streams do not agree with one another and no parameters
 * come out.  dir_mano_para_smooth_step filters where a hand is a hand -- the root rotation on SO(3), the 15 finger joints per joint in
 * axis-angle, the frame camera as three scalars, ONE shape per sequence -- and regenerates the mesh, the joints and the 2-D joints from the
 * filtered parameters with the MANO forward, in the same launch.  The rule is restated in torch (float64 and float32) by
 * tests/helpers/para_smooth_ref.py.  One call is one frame of B sequences x `hands` (1 or 2); one 256-lane workgroup per (sequence, hand); the
 * state is updated in place; no atomics, no workspace, no host read; capturable in a graph.
 *
 * Per hand (dir_mano_para_smooth_hand; every pointer a device pointer):
 *   para           [B,64]  the layout of pd_mano_para_*: 6D root | 45 PCA coefficients | 10 betas | 3 crop-camera values.  Components 61:64 are
 *                          NOT read: the crop moves between frames, the frame does not, so the camera comes in as
 *   cam_px         [B,3]   frame_camera's (scale_px, trans_px x, trans_px y)
 *   raw_verts [B,778,3], raw_joints [B,21,3], raw_joints_px [B,21,2]   optional (NULL): the unfiltered streams, for the raw side of the measures only
 *   smoothed       [B,64]  six | a_y [45] | b_y [10] | c_y [3].  This is NOT a pd_mano_para: 6:51 are the 45 AXIS-ANGLE components with hands_mean
 *                          included (not PCA coefficients), and 61:64 are FRAME pixels (not the crop camera).  six and b_y may be fed to
 *                          dir_mano_forward as they are: six reproduces the R_y the kernel used bit for bit.
 *   verts [B,778,3], joints [B,21,3], joints_px [B,21,2]   the forward at the filtered parameters;  updated int32 [B]: 0, 1 or 2 as below
 *   state          B rows of dir_mano_para_smooth_state_bytes(offsets) bytes, 16-byte aligned, zeroed by the caller before the first frame; rows
 *                  are per (sequence, hand), and the first B rows of a larger state are the state of a smaller batch (sequences end from the tail)
 * valid int32 [B] or NULL is shared by the hands.  tables_host / hands_host: HOST arrays of `hands` entries, passed to the kernel by value.
 *
 * State row: offsets[DIR_MANO_PARA_SMOOTH_FIELDS] (or NULL) receives the byte offsets of
 *   measures  double [8]: raw, filtered sums of mesh_xyz | joint_xyz | joints_px jitter | bone flicker
 *   y1, y2    float32 [2440] each: the last two outputs, verts [2334] | joints [63] | joints_px [42] | pad;   x1, x2: the same of the raw streams
 *   prev      float32 [64]: the last `smoothed`, with the running mean of the betas in 51:61
 *   vel       float32 [64]: the speed estimates -- w^ in 0:3, the fingers' in 6:51, the camera's in 61:64, the rest 0
 *   n_shape, age, run, count   int32: usable frames averaged into the shape; frames since the last update (0 = never initialised, saturating);
 *             consecutive updates; frames counted into the measures
 * dir_mano_para_smooth_state_bytes is a pure host function and returns the row size.
 *
 * Per row, in this order.  Float32 arithmetic, every operation rounded on its own (`fp contract` is OFF in step 0's root matrix, in steps 4 and 5 and in
 * the Rodrigues routine; it is the compiler's default, as in mano.hip, in the PCA product and in step 6 outside Rodrigues); sums of three products are
 * ((p0 + p1) + p2); dt, 2 pi dt and alpha(d_cutoff) are computed in double and rounded once, as in dir_one_euro_step.
 *   0. inputs, exactly as mano_forward_kernel forms them: R_x = the robust-6D root matrix of para[0:6] and its reflection flag (det < 0);
 *      a_x[45] = hands_mean + comps . para[6:51] (one fmaf chain per component, k ascending); b_x = para[51:61]; c_x = cam_px.
 *   1. usable iff valid is NULL or valid[b] != 0, the 61 components read and the 3 camera values are finite, and R_x is not a reflection.
 *   2. not usable: (R_y, a_y, b_y, c_y) = (R_x, a_x, b_x, c_x) and six = para[0:6] bit for bit, so the forward output is dir_mano_forward's at
 *      para (a NaN propagates); age += 1 if age > 0; run = 0; updated = 0; nothing else in the state changes.
 *   3. initialise, when usable and age == 0 or age > max_gap (or the break of step 4): R_y = R_x with six = para[0:6], a_y = a_x, c_y = c_x;
 *      every speed estimate = 0; age = 1, run = 1, updated = 2; shape as in step 5.
 *   4. update.  dt = age / fps, alpha(fc) = 1 / (1 + 1 / ((2 pi dt) fc)).
 *      root:    R_y1 = robust6D(prev six) (the same routine: the bits of the last frame's R_y);  D = R_y1^T R_x, D_ij = sum_k R_y1[k][i] R_x[k][j];
 *               s = 0.5 (D21 - D12, D02 - D20, D10 - D01);  c = 0.5 (((D00 + D11) + D22) - 1);  n = sqrt((s0 s0 + s1 s1) + s2 s2).
 *               n <= 1e-6 and c < 0: the relative rotation is about pi and its axis undetermined -- the row is a BREAK and goes to step 3.
 *               w = s when n <= 1e-6, else k s with k = atan2(n, c) / n.
 *               per component dx = w / dt, w^ = w^ + alpha(d_cutoff) (dx - w^);  v2 = ((0 + w^0 w^0) + w^1 w^1) + w^2 w^2;
 *               fc = min_cutoff + beta (rot_speed_scale sqrt(v2));  E = the forward's Rodrigues-by-quaternion routine at v = alpha(fc) w (each
 *               component multiplied first) WITHOUT its 1e-8 offset: angle = sqrt((v0 v0 + v1 v1) + v2 v2), E = I when that is 0 (the offset
 *               would turn every step by 1e-8 rad about a fixed direction: the step response would not be the scalar filter's, nor the
 *               rule equivariant);  R_tmp = R_y1 E;  six = columns 0 and 1 of R_tmp;  R_y = robust6D(six).
 *               The state keeps six, not a matrix: the stored rotation cannot drift from orthonormal.
 *      fingers: a is 15 points of 3 components under dir_one_euro_step's step 4 (one cutoff per joint), speed scale rot_speed_scale.
 *      camera:  c is 3 points of 1 component under the same rule, speed scale cam_speed_scale.
 *      then age = 1, run += 1 (saturating), updated = 1.
 *   5. shape, on every usable row (initialising or updating; a gap never resets it, only zeroing the state does).  shape_frames == 0: b_y = b_x.
 *      Otherwise, while n_shape < shape_frames: n_shape += 1; mean = b_x when n_shape == 1, else mean = mean + (b_x - mean) / n_shape;
 *      and b_y = mean on every such row.  After shape_frames usable frames the mean is frozen: the betas that leave are the same bits every frame.
 *   6. forward from (R_y, a_y, b_y): mano_forward_kernel's operations from its shape blend and Rodrigues stage on, with the tables' side, center_idx
 *      and root_palm -> verts V, joints J (centred);  joints_px[j] = c_y[0] * J[j].xy + c_y[1:3].  With steps 2, 3 and 5 the first usable frame
 *      of a sequence gives dir_mano_forward's verts and joints bit for bit (at any shape_frames: the mean of one frame is that frame).
 *   7. measures, when run >= 3 after the update, in double (exact from the float32 values), per-lane partials in point order and then a fixed
 *      tree: the second-difference jitter of dir_one_euro_step's step 5, raw (x = the raw_* stream; a NULL stream's sum stays 0) and filtered
 *      (y = the outputs), for mesh_xyz, joint_xyz and joints_px;  bone flicker = sum over the 20 bones of | |J_c - J_p|_t - |J_c - J_p|_{t-1} |,
 *      raw and filtered, the bones of finger f = 0..4 in output joint order being (0, 1+4f), (1+4f, 2+4f), (2+4f, 3+4f), (3+4f, 4+4f);  count += 1.
 *   8. history shift on every usable row: y2 = y1, y1 = y, and per raw stream given x2 = x1, x1 = x.
 * A (sequence, hand) gives the same bits in any slot of any batch and in either hand slot.
 * A null pointer (valid and raw_* aside), B outside 1..DIR_CROP_MAX_BATCH, hands outside 1..2, fps, min_cutoff or d_cutoff <= 0, beta < 0,
 * max_gap < 1, shape_frames < 0 or a negative speed scale gives DIR_E_INVALID and a message before any launch. */
#define DIR_MANO_PARA_SMOOTH_FIELDS 11
typedef struct dir_mano_para_smooth_hand {
    const float* para;          /* [B,64]                                   */
    const float* cam_px;        /* [B,3]                                    */
    const float* raw_verts;     /* [B,778,3] or NULL                        */
    const float* raw_joints;    /* [B,21,3] or NULL                         */
    const float* raw_joints_px; /* [B,21,2] or NULL                         */
    float* smoothed;            /* [B,64]: NOT a pd_mano_para (see above)   */
    float* verts;               /* [B,778,3]                                */
    float* joints;              /* [B,21,3]                                 */
    float* joints_px;           /* [B,21,2]                                 */
    int32_t* updated;           /* [B]                                      */
    void* state;                /* B rows, in and out                       */
} dir_mano_para_smooth_hand;
typedef struct dir_mano_para_smooth_opts {
    double fps, min_cutoff, beta, d_cutoff;
    double rot_speed_scale;     /* rad/s -> the speed unit of beta (100: a guess of 100 mm per radian) */
    double cam_speed_scale;
    int32_t max_gap, shape_frames;
} dir_mano_para_smooth_opts;
long long dir_mano_para_smooth_state_bytes(long long* offsets);
int dir_mano_para_smooth_step(const dir_mano_tables* tables_host, const dir_mano_para_smooth_hand* hands_host, const int32_t* valid,
                              const dir_mano_para_smooth_opts* opts_host, int hands, int B, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* DIR_HIP_H */
