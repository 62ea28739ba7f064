// SURVEY 8f rank 2 (optimiser half): train.py:227 `optim.AdamW(model.parameters(), cfg.lr)` as ONE launch over a flat parameter
// store.  MI355X-first layout: all 92.7 M parameters, their gradients and the two moment buffers live in four contiguous fp32
// buffers (the model's tensors are views into the first), so the step is a single 16-byte-vectorised streaming kernel --
// 4 reads + 3 writes x 4 B per parameter = 2.6 GB per step, HBM-bound -- instead of 963 tensors x 6 elementwise launches, and the
// flat gradient buffer is exactly the bucket a data-parallel all-reduce wants.
// Arithmetic = torch.optim.AdamW's single-tensor update (decoupled weight decay, bias-corrected moments), fp32, in its operation
// order: p *= 1 - lr wd;  m = m + (g - m)(1 - b1);  v = b2 v + (1 - b2) g g;  p -= (lr / bc1) * m / (sqrt(v) / sqrt(bc2) + eps).
#include "dir_common.h"

namespace dir {
namespace {

struct AdamArgs {
    float* p; const float* g; float* m; float* v;
    long long n;
    float decay, w1, beta2, w2, bc2_sqrt, eps, step_size;
};

__device__ __forceinline__ void adam1(float& p, float g, float& m, float& v, const AdamArgs& a) {
#pragma clang fp contract(off)
    p = p * a.decay;
    m = m + a.w1 * (g - m);                         // exp_avg.lerp_(grad, 1 - beta1)
    v = v * a.beta2 + (a.w2 * g) * g;               // exp_avg_sq.mul_(beta2).addcmul_(grad, grad, value=1 - beta2): value * t1 * t2
    const float denom = sqrtf(v) / a.bc2_sqrt + a.eps;
    p = p - a.step_size * (m / denom);              // param.addcdiv_(exp_avg, denom, value=-step_size)
}

__global__ __launch_bounds__(256) void adamw_kernel(AdamArgs a) {
    const long long n4 = a.n >> 2;
    const long long stride = (long long)gridDim.x * blockDim.x;
    typedef float v4 __attribute__((ext_vector_type(4)));
    for (long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x; i < n4; i += stride) {
        // every byte is touched once per step and the four buffers (1.5 GB) exceed every cache: non-temporal loads / stores
        v4 p = __builtin_nontemporal_load(reinterpret_cast<v4*>(a.p) + i);
        const v4 g = __builtin_nontemporal_load(reinterpret_cast<const v4*>(a.g) + i);
        v4 m = __builtin_nontemporal_load(reinterpret_cast<v4*>(a.m) + i);
        v4 v = __builtin_nontemporal_load(reinterpret_cast<v4*>(a.v) + i);
#pragma unroll
        for (int e = 0; e < 4; ++e) {
            float pe = p[e], me = m[e], ve = v[e];
            adam1(pe, g[e], me, ve, a);
            p[e] = pe; m[e] = me; v[e] = ve;
        }
        __builtin_nontemporal_store(p, reinterpret_cast<v4*>(a.p) + i);
        __builtin_nontemporal_store(m, reinterpret_cast<v4*>(a.m) + i);
        __builtin_nontemporal_store(v, reinterpret_cast<v4*>(a.v) + i);
    }
    if (blockIdx.x == 0 && threadIdx.x < (a.n & 3)) {            // tail (n not a multiple of 4)
        const long long i = (n4 << 2) + threadIdx.x;
        float p = a.p[i], m = a.m[i], v = a.v[i];
        adam1(p, a.g[i], m, v, a);
        a.p[i] = p; a.m[i] = m; a.v[i] = v;
    }
}

// ---- the guarded step (include/dir_hip.h, "guarded AdamW step"): global gradient norm -> decision on the device -> clipped update + EMA
constexpr int kNormBlock = 256;
constexpr int kNormMaxBlocks = 256 * 16;                          // as adamw_kernel's grid: 16 workgroups per CU, grid-stride beyond

inline long long norm_blocks(long long n) {
    long long blocks = ((n >> 2) + kNormBlock - 1) / kNormBlock;
    if (blocks > kNormMaxBlocks) blocks = kNormMaxBlocks;
    return blocks < 1 ? 1 : blocks;
}

// fixed tree over the workgroup's 256 doubles: the same operands meet in the same order on every run
__device__ __forceinline__ double block_sum_256(double x, double* sh) {
    sh[threadIdx.x] = x;
    __syncthreads();
#pragma unroll
    for (int s = kNormBlock / 2; s > 0; s >>= 1) {
        if ((int)threadIdx.x < s) sh[threadIdx.x] += sh[threadIdx.x + s];
        __syncthreads();
    }
    return sh[0];
}

// stage one: partial[blockIdx.x] = sum over this workgroup's grid-stride share of (double)g * (double)g
__global__ __launch_bounds__(kNormBlock) void grad_sumsq_partial_kernel(const float* __restrict__ g, long long n, double* __restrict__ partial) {
    __shared__ double sh[kNormBlock];
    const long long n4 = n >> 2;
    const long long stride = (long long)gridDim.x * blockDim.x;
    typedef float v4 __attribute__((ext_vector_type(4)));
    double a0 = 0.0, a1 = 0.0, a2 = 0.0, a3 = 0.0;
    for (long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x; i < n4; i += stride) {
        const v4 x = reinterpret_cast<const v4*>(g)[i];           // plain loads: the update reads the gradient again right after
        const double d0 = x[0], d1 = x[1], d2 = x[2], d3 = x[3];
        a0 += d0 * d0; a1 += d1 * d1; a2 += d2 * d2; a3 += d3 * d3;
    }
    double acc = (a0 + a1) + (a2 + a3);
    if (blockIdx.x == 0 && (long long)threadIdx.x < (n & 3)) {   // tail (n not a multiple of 4)
        const double d = g[(n4 << 2) + threadIdx.x];
        acc += d * d;
    }
    const double s = block_sum_256(acc, sh);
    if (threadIdx.x == 0) partial[blockIdx.x] = s;
}

struct GuardArgs {
    const double* partial; int n_partial;
    dir_guard_state* st;
    double max_norm, beta1, beta2;
    int skip_nonfinite;
};

// stage two and the decision: one workgroup; thread t sums partials t, t + 256, ... in index order, then the fixed tree
__global__ __launch_bounds__(kNormBlock) void grad_guard_decide_kernel(GuardArgs a) {
    __shared__ double sh[kNormBlock];
    double acc = 0.0;
    for (int i = threadIdx.x; i < a.n_partial; i += kNormBlock) acc += a.partial[i];
    const double sumsq = block_sum_256(acc, sh);
    if (threadIdx.x != 0) return;
    dir_guard_state s = *a.st;
    s.sumsq = sumsq;
    s.norm = sqrt(sumsq);
    s.nonfinite = isfinite(sumsq) ? 0 : 1;
    const double c = a.max_norm / (s.norm + 1e-6);              // torch.nn.utils.clip_grad_norm_
    s.coef = (float)(c < 1.0 ? c : 1.0);                         // a NaN norm (not skipped) leaves the gradient as it is: it is poison already
    s.skip = (a.skip_nonfinite && s.nonfinite) ? 1 : 0;
    if (s.skip) {
        s.skipped += 1;
        s.skipped_in_row += 1;
    } else {
        s.applied += 1;
        s.skipped_in_row = 0;
        if (s.coef < 1.0f) s.clipped += 1;
        // dir_adamw_step's host prefactors for step = applied, in double
        s.bc1 = 1.0 - pow(a.beta1, (double)s.applied);
        s.bc2_sqrt = (float)sqrt(1.0 - pow(a.beta2, (double)s.applied));
    }
    *a.st = s;
}

struct GuardedAdamArgs {
    AdamArgs a;                                                   // bc2_sqrt and step_size are filled per thread from the device state
    float* e;                                                     // EMA store or nullptr
    float ema_w, ema_1mw;                                         // (float)(1 - decay), 1.0f - ema_w
    double lr;
    const dir_guard_state* st;
};

// torch's lerp_(p, w): e + w (p - e) for w < 0.5, p - (p - e)(1 - w) otherwise (so that w = 1 returns p itself)
__device__ __forceinline__ float ema1(float e, float p, float w, float omw) {
#pragma clang fp contract(off)
    const float d = p - e;
    return w < 0.5f ? e + w * d : p - d * omw;
}

__device__ __forceinline__ float scaled(float g, float coef) {
#pragma clang fp contract(off)
    return g * coef;                                              // g.mul_(coef) before the update, as clip_grad_norm_ leaves it
}

template <bool EMA>
__global__ __launch_bounds__(256) void adamw_guarded_kernel(GuardedAdamArgs ga) {
    const dir_guard_state* st = ga.st;
    if (st->skip) return;                                         // a skipped step stores nothing: p, m, v, e keep their bits
    AdamArgs a = ga.a;
    const float coef = st->coef;
    a.bc2_sqrt = st->bc2_sqrt;
    a.step_size = (float)(ga.lr / st->bc1);
    const long long n4 = a.n >> 2;
    const long long stride = (long long)gridDim.x * blockDim.x;
    typedef float v4 __attribute__((ext_vector_type(4)));
    for (long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x; i < n4; i += stride) {
        v4 p = __builtin_nontemporal_load(reinterpret_cast<v4*>(a.p) + i);
        const v4 g = __builtin_nontemporal_load(reinterpret_cast<const v4*>(a.g) + i);
        v4 m = __builtin_nontemporal_load(reinterpret_cast<v4*>(a.m) + i);
        v4 v = __builtin_nontemporal_load(reinterpret_cast<v4*>(a.v) + i);
        v4 ev;
        if (EMA) ev = __builtin_nontemporal_load(reinterpret_cast<v4*>(ga.e) + i);
#pragma unroll
        for (int e = 0; e < 4; ++e) {
            float pe = p[e], me = m[e], ve = v[e];
            adam1(pe, scaled(g[e], coef), me, ve, a);
            p[e] = pe; m[e] = me; v[e] = ve;
            if (EMA) ev[e] = ema1(ev[e], pe, ga.ema_w, ga.ema_1mw);
        }
        __builtin_nontemporal_store(p, reinterpret_cast<v4*>(a.p) + i);
        __builtin_nontemporal_store(m, reinterpret_cast<v4*>(a.m) + i);
        __builtin_nontemporal_store(v, reinterpret_cast<v4*>(a.v) + i);
        if (EMA) __builtin_nontemporal_store(ev, reinterpret_cast<v4*>(ga.e) + i);
    }
    if (blockIdx.x == 0 && threadIdx.x < (a.n & 3)) {            // tail (n not a multiple of 4)
        const long long i = (n4 << 2) + threadIdx.x;
        float p = a.p[i], m = a.m[i], v = a.v[i];
        adam1(p, scaled(a.g[i], coef), m, v, a);
        a.p[i] = p; a.m[i] = m; a.v[i] = v;
        if (EMA) ga.e[i] = ema1(ga.e[i], p, ga.ema_w, ga.ema_1mw);
    }
}

}  // namespace
}  // namespace dir

extern "C" long long dir_grad_norm_workspace_bytes(long long n) {
    return n > 0 ? dir::norm_blocks(n) * (long long)sizeof(double) : -1;
}

extern "C" int dir_grad_guard(const float* grad, long long n, double max_norm, int skip_nonfinite, double beta1, double beta2,
                              void* workspace, long long workspace_bytes, dir_guard_state* state, void* stream) {
    using namespace dir;
    DIR_REQUIRE(grad && workspace && state, "dir_grad_guard: null pointer");
    DIR_REQUIRE(n > 0, "dir_grad_guard: n must be positive");
    DIR_REQUIRE((uintptr_t)grad % 16 == 0 && ((uintptr_t)workspace | (uintptr_t)state) % 8 == 0,
                "dir_grad_guard: grad must be 16-byte aligned, workspace and state 8-byte aligned");
    DIR_REQUIRE(max_norm > 0.0, "dir_grad_guard: max_norm must be positive (+inf = no clipping)");
    const long long blocks = norm_blocks(n);
    DIR_REQUIRE(workspace_bytes >= blocks * (long long)sizeof(double), "dir_grad_guard: workspace too small (%lld bytes, %lld needed)",
                workspace_bytes, blocks * (long long)sizeof(double));
    DIR_LAUNCH(grad_sumsq_partial_kernel, dim3((unsigned)blocks), dim3(kNormBlock), 0, (hipStream_t)stream, grad, n, (double*)workspace);
    GuardArgs a;
    a.partial = (const double*)workspace; a.n_partial = (int)blocks; a.st = state;
    a.max_norm = max_norm; a.beta1 = beta1; a.beta2 = beta2; a.skip_nonfinite = skip_nonfinite ? 1 : 0;
    DIR_LAUNCH(grad_guard_decide_kernel, dim3(1), dim3(kNormBlock), 0, (hipStream_t)stream, a);
    return check_launch("dir_grad_guard");
}

extern "C" int dir_adamw_guarded_step(float* param, const float* grad, float* exp_avg, float* exp_avg_sq, float* ema, long long n, double lr,
                                      double beta1, double beta2, double eps, double weight_decay, double ema_decay,
                                      const dir_guard_state* state, void* stream) {
    using namespace dir;
    DIR_REQUIRE(param && grad && exp_avg && exp_avg_sq && state, "dir_adamw_guarded_step: null pointer");
    DIR_REQUIRE(n > 0, "dir_adamw_guarded_step: n must be positive");
    DIR_REQUIRE(((uintptr_t)param | (uintptr_t)grad | (uintptr_t)exp_avg | (uintptr_t)exp_avg_sq | (uintptr_t)ema) % 16 == 0 &&
                    (uintptr_t)state % 8 == 0,
                "dir_adamw_guarded_step: buffers must be 16-byte aligned (state: 8)");
    DIR_REQUIRE(ema_decay >= 0.0 && ema_decay <= 1.0, "dir_adamw_guarded_step: ema_decay must be in [0, 1]");
    GuardedAdamArgs ga;
    AdamArgs& a = ga.a;
    a.p = param; a.g = grad; a.m = exp_avg; a.v = exp_avg_sq; a.n = n;
    a.decay = (float)(1.0 - lr * weight_decay);
    a.w1 = (float)(1.0 - beta1);
    a.beta2 = (float)beta2;
    a.w2 = (float)(1.0 - beta2);
    a.bc2_sqrt = 0.f;
    a.eps = (float)eps;
    a.step_size = 0.f;
    ga.e = ema;
    ga.ema_w = ema ? (float)(1.0 - ema_decay) : 0.f;
    ga.ema_1mw = 1.0f - ga.ema_w;
    ga.lr = lr;
    ga.st = state;
    const long long n4 = n >> 2;
    long long blocks = (n4 + 255) / 256;
    if (blocks > 256 * 16) blocks = 256 * 16;
    if (blocks < 1) blocks = 1;
    if (ema)
        DIR_LAUNCH(adamw_guarded_kernel<true>, dim3((unsigned)blocks), dim3(256), 0, (hipStream_t)stream, ga);
    else
        DIR_LAUNCH(adamw_guarded_kernel<false>, dim3((unsigned)blocks), dim3(256), 0, (hipStream_t)stream, ga);
    return check_launch("dir_adamw_guarded_step");
}

extern "C" int dir_adamw_step(float* param, const float* grad, float* exp_avg, float* exp_avg_sq, long long n, double lr,
                              double beta1, double beta2, double eps, double weight_decay, long long step, void* stream) {
    using namespace dir;
    DIR_REQUIRE(param && grad && exp_avg && exp_avg_sq, "dir_adamw_step: null pointer");
    DIR_REQUIRE(n > 0 && step >= 1, "dir_adamw_step: n and step must be positive");
    DIR_REQUIRE(((uintptr_t)param | (uintptr_t)grad | (uintptr_t)exp_avg | (uintptr_t)exp_avg_sq) % 16 == 0,
                "dir_adamw_step: buffers must be 16-byte aligned");
    // scalar prefactors exactly as torch computes them on the host (python doubles), then rounded to the tensors' dtype
    const double bc1 = 1.0 - pow(beta1, (double)step), bc2 = 1.0 - pow(beta2, (double)step);
    AdamArgs a;
    a.p = param; a.g = grad; a.m = exp_avg; a.v = exp_avg_sq; a.n = n;
    a.decay = (float)(1.0 - lr * weight_decay);
    a.w1 = (float)(1.0 - beta1);
    a.beta2 = (float)beta2;
    a.w2 = (float)(1.0 - beta2);
    a.bc2_sqrt = (float)sqrt(bc2);
    a.eps = (float)eps;
    a.step_size = (float)(lr / bc1);
    const long long n4 = n >> 2;
    long long blocks = (n4 + 255) / 256;
    if (blocks > 256 * 16) blocks = 256 * 16;                 // 16 workgroups per CU, grid-stride beyond
    if (blocks < 1) blocks = 1;
    DIR_LAUNCH(adamw_kernel, dim3((unsigned)blocks), dim3(256), 0, (hipStream_t)stream, a);
    return check_launch("dir_adamw_step");
}
