// Backward of the novel-light re-shade (shade_kernel of ra_trace.hip in ra_reshade's configuration: tonemapping = 1, only_visibility = 0,
// vis_shade_map = 0) with respect to albedo, roughness and the probes (gfx950).
//
//   reference: render_human          lib/networks/renderer/novel_light_sphere_tracing.py:21-66 under torch autograd
//              relighting stage      lib/train/trainers/relight_trainer.py:113-118 (geometry frozen, visibility under no_grad:
//                                    sphere_tracing_renderer.py:265; the image loss reaches albedo, roughness and the probe only)
//
//   lin[q,p,c] = sum_l brdf[p,l,c] lvis[p,l] area[l] Lr[q,l,p,c],  rgb = srgb(lin);  given d_rgb:
//   d_albedo[p,c]  = sum_q g[q,p,c] sum_l clip(l.n)/pi lvis area Lr                      (Lambert term only; 0 under glossy_only)
//   d_roughness[p] = sum_q sum_c g[q,p,c] sum_l d glossy / d rough lvis area Lr          (through a2 = rough^4 in D and G; 0 under lambert_only)
//   d_probes[q,y,x,c] = sum_p sum_l sum_taps w_tap brdf[p,l,c] lvis area g[q,p,c]        (sample_probe's bilinear taps, transposed)
//   with g = d_rgb srgb'(lin).  surf, norm, ray_o, lvis and ldot are constants.
//
// Gradient conventions are torch autograd's on the reference's program text: the sRGB clip passes gradient for 0 <= lin <= 1 only
// (slope 12.92 up to 0.0031308, else the derivative of 1.055 (lin + 1e-7)^(1/2.4)); an operand that safe_divide clamps in place gets
// no gradient, nor does a quotient it replaces (NaN / inf) or clips; chi factors and the clips of l.n / v.n are constants.
//
// Shape.  The forward's mapping is kept: one wave per pixel, lanes striding over the lights, the BRDF and its roughness derivative once
// per (pixel, light) for all probes of the launch.  A wave first sums lin like the forward does (same helpers, same expressions, same
// shuffle order), then walks the lights again with g in registers.  d_albedo and d_roughness reduce by wave shuffles in a fixed order.
// d_probes is a scatter of P x L x 4 taps into ph x pw x 3 floats per probe: it is accumulated in an LDS tile of the launch's probes per
// workgroup (16 x 32 x 3 fp32 = 6 KB per probe: 8 probes per launch; 32 x 64: 2 per launch), written out as one partial slab per workgroup
// and summed over the workgroups in index order by slab_sum_kernel — no global float atomics.
//
// Reproducibility.  Every sum has a fixed order.  A workgroup is BW_WAVES waves that walk their pixels in lockstep; they add their taps to
// the tile one wave after the other (a barrier between them), so a tile receives its adds in (pixel, light block) order whatever the
// timing.  Within one LDS add instruction, lanes that hit the same tap are serialised by the LDS unit in lane order.  The grid and the
// pixel -> workgroup map depend on P alone, not on the number of probes: a probe's gradient is bit-identical whether it is computed
// alone or beside others, and from run to run.
#include "ra_kernels.hpp"
#include "ra_shade_dev.hpp"

namespace {

constexpr int BW_WAVES = 4;                 // waves per workgroup (one pixel each per round)
constexpr int BW_TPB = 64 * BW_WAVES;
constexpr int BW_MAXP = 8;                  // probes per launch at most, like the forward

// safe_div that also reports what autograd needs: a_free / b_free = the operand was not clamped, pass = the quotient was neither
// replaced (NaN, inf) nor clipped
__device__ __forceinline__ float safe_div_g(float& a, float& b, bool& a_free, bool& b_free, bool& pass) {
    const float eps = 1e-8f;
    a_free = b_free = true;
    if (a < eps && a >= 0.f) { a = eps; a_free = false; }
    if (a > -eps && a <= 0.f) { a = -eps; a_free = false; }
    if (b < eps && b >= 0.f) { b = eps; b_free = false; }
    if (b > -eps && b <= 0.f) { b = -eps; b_free = false; }
    float d = a / b;
    pass = true;
    if (d != d) { d = 0.f; pass = false; }
    if (isinf(d)) { d = 0.f; pass = false; }
    if (d < -1e10f || d > 1e10f) pass = false;
    return fminf(fmaxf(d, -1e10f), 1e10f);
}

// mf_light's glossy term with its derivative with respect to a2 = rough^4 (D: _get_d :598-608, G: _get_g :580-595), and clip(l.n)
struct MfGrad { float glossy, dgl_da2, l_dot_n; };
__device__ __forceinline__ MfGrad mf_light_grad(const MfView& m, float tan_v_sq, const float p2l[3], const ra_config& cfg) {
    MfGrad r;
    float pl[3] = {p2l[0], p2l[1], p2l[2]};
    fnormalize(pl);
    r.l_dot_n = fminf(fmaxf(pl[0] * m.n[0] + pl[1] * m.n[1] + pl[2] * m.n[2], 1e-4f), 1.f);
    float hv[3] = {pl[0] + m.v[0], pl[1] + m.v[1], pl[2] + m.v[2]};
    fnormalize(hv);
    const float omc5 = 1.f - (pl[0] * hv[0] + pl[1] * hv[1] + pl[2] * hv[2]);
    const float f = cfg.fresnel_f0 + (1.f - cfg.fresnel_f0) * (omc5 * omc5 * omc5 * omc5 * omc5);
    // D = a2 chi / (pi cms^2 (a2 + tan^2)^2)
    const float cos_m = hv[0] * m.n[0] + hv[1] * m.n[1] + hv[2] * m.n[2];
    const float chi_d = cos_m > 0.f ? 1.f : 0.f;
    float cms = cos_m * cos_m;
    float omc = 1.f - cms;
    const float tan_m_sq = safe_div(omc, cms);          // clamps cms in place
    const float at = m.a2 + tan_m_sq;
    float dden = PI_F * (cms * cms) * (at * at);
    float dnum = m.a2 * chi_d;
    bool dn_free, dd_free, d_pass;
    const float dd = safe_div_g(dnum, dden, dn_free, dd_free, d_pass);
    float ddd = 0.f;                                     // d D / d a2
    if (d_pass) {
        if (dn_free) ddd += chi_d / dden;
        if (dd_free) ddd -= dnum / (dden * dden) * (PI_F * (cms * cms) * (2.f * at));
    }
    // G = 2 chi / (1 + sqrt(1 + a2 tan_v^2))
    float cos_t = hv[0] * m.v[0] + hv[1] * m.v[1] + hv[2] * m.v[2];
    float cvc = m.cos_v;
    const float dv = safe_div(cos_t, cvc);
    float gnum = (dv > 0.f ? 1.f : 0.f) * 2.f;
    float gden = m.g_den0;
    bool gn_free, gd_free, g_pass;
    const float gg = safe_div_g(gnum, gden, gn_free, gd_free, g_pass);
    float dgg = 0.f;                                     // d G / d a2
    if (g_pass && gd_free) dgg = -gnum / (gden * gden) * (tan_v_sq / (2.f * (m.g_den0 - 1.f)));
    float mnum = f * gg * dd;
    float mden = 4.f * 1.f * fabsf(m.v_dot_n);
    bool mn_free, md_free, m_pass;
    r.glossy = safe_div_g(mnum, mden, mn_free, md_free, m_pass);
    r.dgl_da2 = (m_pass && mn_free) ? f * (dgg * dd + gg * ddd) / mden : 0.f;
    return r;
}

// sample_probe's taps: the same arithmetic up to the weights; tap k of (x0,y0) (x1,y0) (x0,y1) (x1,y1) is texel idx[k] with weight w[k],
// idx[k] < 0 where the forward skips it (x1 = W or y1 = H on the border)
__device__ __forceinline__ void probe_taps(int H, int W, const float d[3], int idx[4], float w[4]) {
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
    auto tap = [&](int k, int xx, int yy, float ww) {
        idx[k] = (xx >= 0 && xx < W && yy >= 0 && yy < H) ? yy * W + xx : -1;
        w[k] = ww;
    };
    tap(0, x0, y0, wx0 * wy0);
    tap(1, x1, y0, wx1 * wy0);
    tap(2, x0, y1, wx0 * wy1);
    tap(3, x1, y1, wx1 * wy1);
}

// d srgb(x) / dx under autograd: clip(0, 1) passes on [0, 1]; where() selects the branch
__device__ __forceinline__ float srgb_grad(float x) {
    if (!(x >= 0.f && x <= 1.f)) return 0.f;
    return (x <= 0.0031308f) ? 12.92f : (1.055f / 2.4f) * powf(x + 1e-7f, 1.f / 2.4f - 1.f);
}

struct ShadeBwdIn {
    const float *ray_o, *surf, *norm, *albedo, *rough;   // P x 3 / P
    const float* lvis;                                    // P x L
    const float *light_xyz, *light_area; int L;
    const float* probes; int n_probes, ph, pw;            // the launch's probes (<= BW_MAXP, and their tiles fit the LDS budget)
    const float* d_rgb;                                   // n_probes x P x 3 (the launch's rows)
    int P, rounds;                                        // rounds = pixels per wave
    int accumulate;                                       // d_albedo / d_rough: add to what an earlier launch of this call wrote
    float *d_albedo, *d_rough;                            // P x 3, P (nullable)
    float* slabs;                                         // gridDim.x x n_probes x (ph pw 3), nullable: no probe gradient wanted
};

__global__ __launch_bounds__(BW_TPB) void shade_bwd_kernel(ShadeBwdIn in, ra_config cfg) {
    extern __shared__ float tile[];                       // n_probes x ph x pw x 3
    const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
    const int tile_n = in.ph * in.pw * 3, tiles_n = in.n_probes * tile_n;
    const bool want_probe = in.slabs != nullptr;
    if (want_probe) {
        for (int i = threadIdx.x; i < tiles_n; i += BW_TPB) tile[i] = 0.f;
        __syncthreads();
    }
    for (int rd = 0; rd < in.rounds; ++rd) {
        // round rd: workgroup b, wave w -> pixel (rd * gridDim.x + b) * BW_WAVES + w; every wave of the grid runs every round (barriers below)
        const int h = (rd * gridDim.x + blockIdx.x) * BW_WAVES + wv;
        const bool live = h < in.P;
        const int hh = live ? h : 0;
        const float sp[3] = {in.surf[3 * hh], in.surf[3 * hh + 1], in.surf[3 * hh + 2]};
        float v[3] = {in.ray_o[3 * hh] - sp[0], in.ray_o[3 * hh + 1] - sp[1], in.ray_o[3 * hh + 2] - sp[2]};
        {   // as shade_kernel: surf2cam = normalize(ray_o - surf), then F.normalize inside Microfacet
            const float nn = sqrtf(v[0] * v[0] + v[1] * v[1] + v[2] * v[2]) + 1e-8f;
            v[0] /= nn; v[1] /= nn; v[2] /= nn;
            fnormalize(v);
        }
        const float nraw[3] = {in.norm[3 * hh], in.norm[3 * hh + 1], in.norm[3 * hh + 2]};
        const float alb[3] = {in.albedo[3 * hh], in.albedo[3 * hh + 1], in.albedo[3 * hh + 2]};
        const float rough = in.rough[hh];
        const MfView mv = mf_view(v, nraw, rough);
        float tan_v_sq;                                   // mf_view's, which it does not keep
        {
            float cvs = fminf(fmaxf(mv.cos_v * mv.cos_v, 0.f), 1.f);
            float one_m = 1.f - cvs;
            tan_v_sq = fminf(fmaxf(safe_div(one_m, cvs), 0.f), 1e10f);
        }
        const float da2_dr = 4.f * rough * rough * rough;

        // pass 1: lin as the forward sums it
        float g[BW_MAXP][3];
#pragma unroll
        for (int q = 0; q < BW_MAXP; ++q) g[q][0] = g[q][1] = g[q][2] = 0.f;
        for (int l = lane; l < in.L; l += 64) {
            float s2l[3] = {in.light_xyz[3 * l] - sp[0], in.light_xyz[3 * l + 1] - sp[1], in.light_xyz[3 * l + 2] - sp[2]};
            {
                const float nn = sqrtf(s2l[0] * s2l[0] + s2l[1] * s2l[1] + s2l[2] * s2l[2]) + 1e-8f;
                s2l[0] /= nn; s2l[1] /= nn; s2l[2] /= nn;
            }
            float brdf[3], sbrdf;
            mf_light(mv, s2l, alb, cfg, brdf, sbrdf);
            const float area = in.light_area[l];
            const float lv = in.lvis[(size_t)hh * in.L + l];
#pragma unroll
            for (int q = 0; q < BW_MAXP; ++q) {
                if (q < in.n_probes) {
                    float Lr[3];
                    sample_probe(in.probes + (size_t)q * in.ph * in.pw * 3, in.ph, in.pw, s2l, Lr);
#pragma unroll
                    for (int c = 0; c < 3; ++c) {
                        const float sh = lv * 1.f * area * Lr[c];
                        g[q][c] += brdf[c] * sh;
                    }
                }
            }
        }
#pragma unroll
        for (int q = 0; q < BW_MAXP; ++q) {
            if (q < in.n_probes) {
#pragma unroll
                for (int c = 0; c < 3; ++c) {
                    float a = g[q][c];
#pragma unroll
                    for (int o = 32; o > 0; o >>= 1) a += __shfl_xor(a, o);
                    const float dr = live ? in.d_rgb[((size_t)q * in.P + hh) * 3 + c] : 0.f;
                    g[q][c] = dr * srgb_grad(a);          // g = d loss / d lin
                }
            }
        }

        // pass 2: the lights again, with g
        float da[3] = {0.f, 0.f, 0.f}, drg = 0.f;
        for (int l0 = 0; l0 < in.L; l0 += 64) {
            const int l = l0 + lane;
            const bool on = live && l < in.L;
            int tidx[4] = {-1, -1, -1, -1};
            float tw[4] = {0.f, 0.f, 0.f, 0.f};
            float coef[3] = {0.f, 0.f, 0.f};              // brdf[c] lvis area
            if (on) {
                float s2l[3] = {in.light_xyz[3 * l] - sp[0], in.light_xyz[3 * l + 1] - sp[1], in.light_xyz[3 * l + 2] - sp[2]};
                {
                    const float nn = sqrtf(s2l[0] * s2l[0] + s2l[1] * s2l[1] + s2l[2] * s2l[2]) + 1e-8f;
                    s2l[0] /= nn; s2l[1] /= nn; s2l[2] /= nn;
                }
                const MfGrad mg = mf_light_grad(mv, tan_v_sq, s2l, cfg);
                const float la = in.lvis[(size_t)hh * in.L + l] * in.light_area[l];
                probe_taps(in.ph, in.pw, s2l, tidx, tw);
                const float lam_c = cfg.glossy_only ? 0.f : mg.l_dot_n / PI_F * la;          // d brdf[c] / d albedo[c] (times lvis area)
                const float gl_c = cfg.lambert_only ? 0.f : mg.dgl_da2 * da2_dr * la;         // d brdf[c] / d rough
#pragma unroll
                for (int c = 0; c < 3; ++c) {
                    const float lam = alb[c] / PI_F * mg.l_dot_n;
                    coef[c] = (cfg.lambert_only ? lam : (cfg.glossy_only ? mg.glossy : mg.glossy + lam)) * la;
                }
#pragma unroll
                for (int q = 0; q < BW_MAXP; ++q) {
                    if (q < in.n_probes) {
                        const float* img = in.probes + (size_t)q * in.ph * in.pw * 3;
                        float Lr[3] = {0.f, 0.f, 0.f};
#pragma unroll
                        for (int k = 0; k < 4; ++k)
                            if (tidx[k] >= 0) {
                                const float* p = img + (size_t)tidx[k] * 3;
                                Lr[0] += tw[k] * p[0]; Lr[1] += tw[k] * p[1]; Lr[2] += tw[k] * p[2];
                            }
#pragma unroll
                        for (int c = 0; c < 3; ++c) {
                            const float gl = g[q][c] * Lr[c];
                            da[c] += lam_c * gl;
                            drg += gl_c * gl;
                        }
                    }
                }
            }
            if (want_probe) {
                // the waves of the workgroup add to the tile one after the other: the tile sees (pixel, light block) order
                for (int t = 0; t < BW_WAVES; ++t) {
                    if (t == wv && on) {
#pragma unroll
                        for (int q = 0; q < BW_MAXP; ++q) {
                            if (q < in.n_probes) {
                                float* tq = tile + q * tile_n;
#pragma unroll
                                for (int k = 0; k < 4; ++k)
                                    if (tidx[k] >= 0) {
#pragma unroll
                                        for (int c = 0; c < 3; ++c) atomicAdd(tq + tidx[k] * 3 + c, tw[k] * (coef[c] * g[q][c]));
                                    }
                            }
                        }
                    }
                    __syncthreads();
                }
            }
        }
#pragma unroll
        for (int o = 32; o > 0; o >>= 1) {
            da[0] += __shfl_xor(da[0], o); da[1] += __shfl_xor(da[1], o); da[2] += __shfl_xor(da[2], o);
            drg += __shfl_xor(drg, o);
        }
        if (live && lane == 0) {
            if (in.d_albedo) {
#pragma unroll
                for (int c = 0; c < 3; ++c) in.d_albedo[3 * h + c] = in.accumulate ? in.d_albedo[3 * h + c] + da[c] : da[c];
            }
            if (in.d_rough) in.d_rough[h] = in.accumulate ? in.d_rough[h] + drg : drg;
        }
    }
    if (want_probe) {
        __syncthreads();
        float* slab = in.slabs + (size_t)blockIdx.x * tiles_n;
        for (int i = threadIdx.x; i < tiles_n; i += BW_TPB) slab[i] = tile[i];
    }
}

// out[i] = sum over the G slabs, in slab order (four interleaved partial sums, combined in a fixed order)
__global__ __launch_bounds__(256) void slab_sum_kernel(const float* __restrict__ slabs, int G, int n, float* __restrict__ out) {
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i >= n) return;
    float a0 = 0.f, a1 = 0.f, a2 = 0.f, a3 = 0.f;
    int b = 0;
    for (; b + 4 <= G; b += 4) {
        a0 += slabs[(size_t)b * n + i];
        a1 += slabs[(size_t)(b + 1) * n + i];
        a2 += slabs[(size_t)(b + 2) * n + i];
        a3 += slabs[(size_t)(b + 3) * n + i];
    }
    for (; b < G; ++b) a0 += slabs[(size_t)b * n + i];
    out[i] = (a0 + a1) + (a2 + a3);
}

}  // namespace

int shade_bwd_grid(int P) {
    const int wgs = (P + BW_WAVES - 1) / BW_WAVES;
    return wgs < SHADE_BWD_MAX_GRID ? wgs : SHADE_BWD_MAX_GRID;
}

int shade_bwd_probes_per_launch(int ph, int pw) {
    const size_t tile_bytes = (size_t)ph * pw * 3 * sizeof(float);
    const size_t fit = SHADE_BWD_LDS_BYTES / tile_bytes;
    return (int)(fit < (size_t)BW_MAXP ? fit : (size_t)BW_MAXP);
}

void launch_shade_bwd(const ShadeBwd& a, const ra_config& cfg, hipStream_t s) {
    if (a.P <= 0 || a.n_probes <= 0) return;
    const int G = shade_bwd_grid(a.P);
    const int per = shade_bwd_probes_per_launch(a.ph, a.pw);
    const size_t tile_n = (size_t)a.ph * a.pw * 3;
    for (int q0 = 0; q0 < a.n_probes; q0 += per) {
        const int nq = a.n_probes - q0 < per ? a.n_probes - q0 : per;
        ShadeBwdIn in{};
        in.ray_o = a.ray_o; in.surf = a.surf; in.norm = a.norm; in.albedo = a.albedo; in.rough = a.rough; in.lvis = a.lvis;
        in.light_xyz = a.light_xyz; in.light_area = a.light_area; in.L = a.L;
        in.probes = a.probes + q0 * tile_n; in.n_probes = nq; in.ph = a.ph; in.pw = a.pw;
        in.d_rgb = a.d_rgb + (size_t)q0 * a.P * 3;
        in.P = a.P; in.rounds = (a.P + G * BW_WAVES - 1) / (G * BW_WAVES);
        in.accumulate = q0 > 0;
        in.d_albedo = a.d_albedo; in.d_rough = a.d_rough;
        in.slabs = a.d_probes ? a.slabs : nullptr;
        if (!in.d_albedo && !in.d_rough && !in.slabs) return;
        const size_t lds = in.slabs ? nq * tile_n * sizeof(float) : 0;
        hipLaunchKernelGGL(shade_bwd_kernel, dim3(G), dim3(BW_TPB), lds, s, in, cfg);
        if (in.slabs) {
            const int n = (int)(nq * tile_n);
            hipLaunchKernelGGL(slab_sum_kernel, dim3((n + 255) / 256), dim3(256), 0, s, a.slabs, G, n, a.d_probes + q0 * tile_n);
        }
    }
}
