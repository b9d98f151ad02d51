// Fused global-norm clip + Adam / AdamW (optionally amsgrad) on flat fp32 buffers: torch.nn.utils.clip_grad_norm_ +
// torch.optim.Adam(W).step() of the reference's nnUNetTrainerAdam family (variants/optimizer/nnUNetTrainerAdam.py) in one
// streaming pass.  The arithmetic is torch's single-tensor path (torch/optim/adam.py::_single_tensor_adam).
// HBM-bound: reads p, g, m, v[, vmax] and writes p, m, v[, vmax]: 28 B / parameter, 36 B with amsgrad.  The gradient
// sum of squares comes from mvd_grad_sumsq (sgd.hip).
//
// Scalars: bias correction changes every step, so NO scalar is a kernel argument.  `hyper` is 8 doubles the host writes
// ({lr, beta1, beta2, eps, weight_decay, max_norm, grad_scale, -}) followed by 16 floats the library writes; `step` is an
// int64 counter.  k_adam_scalars (one thread, launched ahead of the update on the same stream) advances the counter and forms
// every fp32 scalar of the update in fp64, rounded once; k_adam reads those floats only, so no thread of a launch reads
// the counter another thread of that launch writes, and an eager step and a replayed one run the same instructions.
#include "common.h"

namespace mvd {

enum { AD_STEP_SIZE = 0, AD_BC2SQRT, AD_DECAY, AD_OMB1, AD_BETA2, AD_OMB2, AD_EPS, AD_WD, AD_MAX_NORM, AD_GSCALE, AD_COUNT };

struct AdamScalars {
    float step_size, bc2sqrt, decay, omb1, beta2, omb2, eps, wd, gscale, clip;
};

__global__ void k_adam_scalars(double *__restrict__ hyper, long long *__restrict__ step) {
#pragma clang fp contract(off)
    if (blockIdx.x != 0 || threadIdx.x != 0) return;
    const long long t = step[0] + 1;
    step[0] = t;
    const double lr = hyper[0], b1 = hyper[1], b2 = hyper[2], eps = hyper[3], wd = hyper[4];
    float *d = reinterpret_cast<float *>(hyper + 8);
    d[AD_STEP_SIZE] = (float)(lr / (1.0 - pow(b1, (double)t)));
    d[AD_BC2SQRT] = (float)sqrt(1.0 - pow(b2, (double)t));
    d[AD_DECAY] = (float)(1.0 - lr * wd);
    d[AD_OMB1] = (float)(1.0 - b1);
    d[AD_BETA2] = (float)b2;
    d[AD_OMB2] = (float)(1.0 - b2);
    d[AD_EPS] = (float)eps;
    d[AD_WD] = (float)wd;
    d[AD_MAX_NORM] = (float)hyper[5];
    d[AD_GSCALE] = (float)hyper[6];
}

// One element.  Every fused multiply-add is an explicit fmaf and nothing else may be contracted, so the result does not
// depend on -ffp-contract; sqrtf and / are the IEEE ones.
template <bool DECOUPLED, bool AMSGRAD>
__device__ inline void adam_one(float &p, float g, float &m, float &v, float &vmax, const AdamScalars &s) {
#pragma clang fp contract(off)
    g = g * s.gscale;  // data-parallel mean (as k_sgd)
    g = g * s.clip;
    if (DECOUPLED) p = p * s.decay;       // AdamW: param.mul_(1 - lr * weight_decay)
    else g = fmaf(s.wd, p, g);            // Adam:  grad.add(param, alpha=weight_decay)
    m = fmaf(s.omb1, g - m, m);           // exp_avg.lerp_(grad, 1 - beta1)
    v = fmaf(s.omb2 * g, g, v * s.beta2); // exp_avg_sq.mul_(beta2).addcmul_(grad, grad, value=1 - beta2)
    float vhat = v;
    if (AMSGRAD) {
        vmax = fmaxf(vmax, v);
        vhat = vmax;
    }
    const float denom = sqrtf(vhat) / s.bc2sqrt + s.eps;
    p = p - (s.step_size * m) / denom;    // param.addcdiv_(exp_avg, denom, value=-step_size)
}

template <bool DECOUPLED, bool AMSGRAD>
__global__ void k_adam(float *__restrict__ p, const float *__restrict__ g, float *__restrict__ m, float *__restrict__ v,
                       float *__restrict__ vmax, const float *__restrict__ sumsq, long n,
                       const float *__restrict__ d) {
#pragma clang fp contract(off)
    AdamScalars s;
    s.step_size = d[AD_STEP_SIZE]; s.bc2sqrt = d[AD_BC2SQRT]; s.decay = d[AD_DECAY]; s.omb1 = d[AD_OMB1];
    s.beta2 = d[AD_BETA2]; s.omb2 = d[AD_OMB2]; s.eps = d[AD_EPS]; s.wd = d[AD_WD]; s.gscale = d[AD_GSCALE];
    const float max_norm = d[AD_MAX_NORM];
    s.clip = 1.0f;
    if (max_norm > 0.f) {
        float total = sqrtf(sumsq[0]) * s.gscale;  // sumsq is over the un-scaled buffer
        s.clip = max_norm / (total + 1e-6f);       // torch.nn.utils.clip_grad_norm_
        if (s.clip > 1.0f) s.clip = 1.0f;
    }
    const long n4 = n / 4;
    float4 *p4 = reinterpret_cast<float4 *>(p);
    const float4 *g4 = reinterpret_cast<const float4 *>(g);
    float4 *m4 = reinterpret_cast<float4 *>(m);
    float4 *v4 = reinterpret_cast<float4 *>(v);
    float4 *x4 = reinterpret_cast<float4 *>(vmax);
    for (long i = (long)blockIdx.x * blockDim.x + threadIdx.x; i < n4; i += (long)gridDim.x * blockDim.x) {
        float4 pp = p4[i], gg = g4[i], mm = m4[i], vv = v4[i], xx = AMSGRAD ? x4[i] : make_float4(0, 0, 0, 0);
        adam_one<DECOUPLED, AMSGRAD>(pp.x, gg.x, mm.x, vv.x, xx.x, s);
        adam_one<DECOUPLED, AMSGRAD>(pp.y, gg.y, mm.y, vv.y, xx.y, s);
        adam_one<DECOUPLED, AMSGRAD>(pp.z, gg.z, mm.z, vv.z, xx.z, s);
        adam_one<DECOUPLED, AMSGRAD>(pp.w, gg.w, mm.w, vv.w, xx.w, s);
        p4[i] = pp;
        m4[i] = mm;
        v4[i] = vv;
        if (AMSGRAD) x4[i] = xx;
    }
    if (blockIdx.x == 0 && threadIdx.x < (int)(n - n4 * 4)) {
        long i = n4 * 4 + threadIdx.x;
        float pp = p[i], mm = m[i], vv = v[i], xx = AMSGRAD ? vmax[i] : 0.f;
        adam_one<DECOUPLED, AMSGRAD>(pp, g[i], mm, vv, xx, s);
        p[i] = pp;
        m[i] = mm;
        v[i] = vv;
        if (AMSGRAD) vmax[i] = xx;
    }
}

}  // namespace mvd

using namespace mvd;

extern "C" {

int mvd_adam_step(float *p, const float *g, float *m, float *v, float *vmax, const float *sumsq, long n, double *hyper,
                  long long *step, int decoupled, void *stream) {
    MVD_REQUIRE(p && g && m && v && sumsq && hyper && step && n > 0, "adam_step: bad arguments");
    MVD_REQUIRE((((uintptr_t)p | (uintptr_t)g | (uintptr_t)m | (uintptr_t)v | (uintptr_t)vmax) & 15) == 0,
                "adam_step: buffers must be 16-byte aligned");
    MVD_REQUIRE((((uintptr_t)hyper | (uintptr_t)step) & 7) == 0, "adam_step: hyper and step must be 8-byte aligned");
    hipStream_t s = as_stream(stream);
    hipLaunchKernelGGL(k_adam_scalars, dim3(1), dim3(1), 0, s, hyper, step);
    if (check_launch("adam_step (scalars)")) return 1;
    long bx = cdiv(n / 4 + 1, 256);
    if (bx > 4096) bx = 4096;
    const float *d = reinterpret_cast<const float *>(hyper + 8);
#define MVD_ADAM_LAUNCH(DEC, AMS) \
    hipLaunchKernelGGL((k_adam<DEC, AMS>), dim3(bx), dim3(256), 0, s, p, g, m, v, vmax, sumsq, n, d)
    if (decoupled) {
        if (vmax) MVD_ADAM_LAUNCH(true, true);
        else MVD_ADAM_LAUNCH(true, false);
    } else {
        if (vmax) MVD_ADAM_LAUNCH(false, true);
        else MVD_ADAM_LAUNCH(false, false);
    }
#undef MVD_ADAM_LAUNCH
    return check_launch("adam_step");
}
}
