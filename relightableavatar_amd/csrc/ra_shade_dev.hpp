// Device helpers of the shading kernels, shared by the forward (ra_trace.hip) and the backward of the re-shade (ra_shade_bwd.hip):
// safe_divide, F.normalize, the equirect probe lookup, linear2srgb and the microfacet BRDF split into its per-pixel and per-light parts.
#pragma once
#include "ra_kernels.hpp"

namespace {

constexpr float PI_F = 3.14159265358979323846f;

// safe_divide with its in-place clamps (relight_utils.py:618-633). a and b are clamped by reference
// because the reference aliases them with tensors it keeps using.
__device__ __forceinline__ float safe_div(float& a, float& b) {
    const float eps = 1e-8f;
    if (a < eps && a >= 0.f) a = eps;
    if (a > -eps && a <= 0.f) a = -eps;
    if (b < eps && b >= 0.f) b = eps;
    if (b > -eps && b <= 0.f) b = -eps;
    float d = a / b;
    if (d != d) d = 0.f;
    if (isinf(d)) d = 0.f;
    return fminf(fmaxf(d, -1e10f), 1e10f);
}

__device__ __forceinline__ void fnormalize(float v[3]) {       // F.normalize(eps=1e-7)
    const float n = fmaxf(sqrtf(v[0] * v[0] + v[1] * v[1] + v[2] * v[2]), 1e-7f);
    v[0] /= n; v[1] /= n; v[2] /= n;
}

// equirect bilinear lookup, align_corners=False, border padding (relight_utils.py:106-127)
__device__ __forceinline__ void sample_probe(const float* __restrict__ img, int H, int W, const float d[3], float out[3]) {
    const float theta = acosf(d[2]) - 1e-6f;
    const float phi = atan2f(d[1], d[0]);
    const float qy = (theta / PI_F) * 2.f - 1.f;
    const float qx = -phi / PI_F;
    float ix = ((qx + 1.f) * W - 1.f) * 0.5f;
    float iy = ((qy + 1.f) * H - 1.f) * 0.5f;
    ix = fminf(fmaxf(ix, 0.f), (float)(W - 1));
    iy = fminf(fmaxf(iy, 0.f), (float)(H - 1));
    const float fx = floorf(ix), fy = floorf(iy);
    const int x0 = (int)fx, y0 = (int)fy, x1 = x0 + 1, y1 = y0 + 1;
    const float wx1 = ix - fx, wy1 = iy - fy, wx0 = 1.f - wx1, wy0 = 1.f - wy1;
    out[0] = out[1] = out[2] = 0.f;
    auto add = [&](int xx, int yy, float w) {
        if (xx >= 0 && xx < W && yy >= 0 && yy < H) {
            const float* p = img + ((size_t)yy * W + xx) * 3;
            out[0] += w * p[0]; out[1] += w * p[1]; out[2] += w * p[2];
        }
    };
    add(x0, y0, wx0 * wy0);
    add(x1, y0, wx1 * wy0);
    add(x0, y1, wx0 * wy1);
    add(x1, y1, wx1 * wy1);
}

__device__ __forceinline__ float srgb(float x) {                // relight_utils.py:179-192
    x = fminf(fmaxf(x, 0.f), 1.f);
    return (x <= 0.0031308f) ? x * 12.92f : 1.055f * powf(x + 1e-7f, 1.f / 2.4f) - (1.055f - 1.f);
}

// Microfacet.__call__ (relight_utils.py:484-577, cancel_cosine = True) split into its per-pixel and per-light parts;
// safe_divide's in-place clamps of its arguments (the aliasing of cos^2 in _get_d / _get_g) are reproduced.
struct MfView { float v[3], n[3], a2, v_dot_n, cos_v, g_den0; };
__device__ __forceinline__ MfView mf_view(const float p2c[3], const float normal[3], float rough) {
    MfView m;
#pragma unroll
    for (int c = 0; c < 3; ++c) { m.v[c] = p2c[c]; m.n[c] = normal[c]; }
    fnormalize(m.v);
    fnormalize(m.n);
    const float alpha = rough * rough;
    m.a2 = alpha * alpha;
    m.v_dot_n = fminf(fmaxf(m.v[0] * m.n[0] + m.v[1] * m.n[1] + m.v[2] * m.n[2], 1e-4f), 1.f);
    // view-only part of G (_get_g :580-595); cos_theta_v is clamped in place by the first safe_divide
    float cos_v = m.n[0] * m.v[0] + m.n[1] * m.v[1] + m.n[2] * m.v[2];
    {
        const float eps = 1e-8f;
        if (cos_v < eps && cos_v >= 0.f) cos_v = eps;
        if (cos_v > -eps && cos_v <= 0.f) cos_v = -eps;
    }
    m.cos_v = cos_v;
    float cvs = fminf(fmaxf(cos_v * cos_v, 0.f), 1.f);
    float one_m = 1.f - cvs;
    float tan_v_sq = safe_div(one_m, cvs);
    tan_v_sq = fminf(fmaxf(tan_v_sq, 0.f), 1e10f);
    m.g_den0 = 1.f + sqrtf(1.f + m.a2 * tan_v_sq);
    return m;
}
// brdf[c] = glossy + albedo/pi * clip(l.n) (or the ablation variants); sbrdf = the albedo-0 value (:740)
__device__ __forceinline__ void mf_light(const MfView& m, const float p2l[3], const float alb[3], const ra_config& cfg, float brdf[3], float& sbrdf) {
    float pl[3] = {p2l[0], p2l[1], p2l[2]};
    fnormalize(pl);
    const float l_dot_n = fminf(fmaxf(pl[0] * m.n[0] + pl[1] * m.n[1] + pl[2] * m.n[2], 1e-4f), 1.f);
    float hv[3] = {pl[0] + m.v[0], pl[1] + m.v[1], pl[2] + m.v[2]};
    fnormalize(hv);
    const float omc5 = 1.f - (pl[0] * hv[0] + pl[1] * hv[1] + pl[2] * hv[2]);
    const float f = cfg.fresnel_f0 + (1.f - cfg.fresnel_f0) * (omc5 * omc5 * omc5 * omc5 * omc5);
    // D (_get_d :598-608)
    const float cos_m = hv[0] * m.n[0] + hv[1] * m.n[1] + hv[2] * m.n[2];
    const float chi_d = cos_m > 0.f ? 1.f : 0.f;
    float cms = cos_m * cos_m;
    float omc = 1.f - cms;
    const float tan_m_sq = safe_div(omc, cms);          // clamps cms in place
    float dden = PI_F * (cms * cms) * ((m.a2 + tan_m_sq) * (m.a2 + tan_m_sq));
    float dnum = m.a2 * chi_d;
    const float dd = safe_div(dnum, dden);
    // G
    float cos_t = hv[0] * m.v[0] + hv[1] * m.v[1] + hv[2] * m.v[2];
    float cvc = m.cos_v;
    const float dv = safe_div(cos_t, cvc);
    float gnum = (dv > 0.f ? 1.f : 0.f) * 2.f;
    float gden = m.g_den0;
    const float gg = safe_div(gnum, gden);
    float mnum = f * gg * dd;
    float mden = 4.f * 1.f * fabsf(m.v_dot_n);
    const float glossy = safe_div(mnum, mden);
#pragma unroll
    for (int c = 0; c < 3; ++c) {
        const float lam = alb[c] / PI_F * l_dot_n;
        brdf[c] = cfg.lambert_only ? lam : (cfg.glossy_only ? glossy : glossy + lam);
    }
    sbrdf = cfg.lambert_only ? 0.f : glossy;
}

}  // namespace
