// SDF features on CANONICAL points (ra_canonical_features): the signed-distance half of K4's forward kernel (ra_k4.hpp,
// mlp_fwd_tape_kernel) on its own.  Implementation header: ra_k4_canon_{f16,bf16}.hip instantiate one kernel each.
//
//   reference: signed_distance_network.feat(cpts + noise)    lib/networks/relight/relight_network.py:107-118
//
// The jitter-smoothness regularisers of the relighting stage evaluate the material heads on the SDF network's features at
// canonical points plus fresh noise, every optimisation step — no residual deformation net in front (the points already ARE
// canonical), no pose condition, no gradient, hence no tape.
//
//   * same code, same bits: the encoding (8 frequencies + hi / lo coordinate columns), the eight softplus layers in the scaled
//     domain and the 256 feature rows are the very templates of ra_k4.hpp with the tape switched off; points are independent
//     MFMA columns, so for cpts = the full query's own fp32 bpts + resd the features equal ra_bigpose_features' bit for bit
//     (tests/test_gpu_relight_reg.py).
//   * no second packed stream: the forward stream (ra_pack.cpp) is [residual net 976 | sdf net 960 | sdf head 16 | feature rows
//     128] fragments of 1 KB.  976 = 61 stages of 16, so the SDF half starts on a stage boundary and this kernel walks
//     fwd_arena + 976 KB as a ring of 69 stages with every fragment at the stage position the full kernel finds it at.
//   * the 16 MFMAs of the head row block stay: their slots carry the pending softplus epilogue of layer 7's last row block, and
//     the stream is consumed in order.  Their result (the distance) is not stored.  1104 of the full kernel's 2080 MFMAs per tile.
#include "ra_k4.hpp"

namespace {

constexpr int CF_SKIP_FRAGS = 976;                     // the residual net's part of the forward stream
constexpr int CF_STAGES = FW_STAGES - CF_SKIP_FRAGS / 16;          // 69
constexpr int CF_BIAS_ROWS = 10;                       // sdf 0..7, head, feature rows
static_assert(CF_SKIP_FRAGS % 16 == 0 && CF_STAGES * 16 == 8 * (4 + 16 * 3 + 20 + 16 * 3) + 16 + 8 * 16, "the SDF half must start on a stage boundary");

template <typename E> struct CfSmem {
    E ring[ST_RING * ST_STAGE_BYTES / 2];
    float bias[CF_BIAS_ROWS * 256];
};

template <typename E, int NW>
__global__ __launch_bounds__(64 * NW, 2) void sdf_feat_kernel(GeoNet net, const void* __restrict__ stream, const float* __restrict__ ba,
                                                                const float* __restrict__ cpts, int n, float* __restrict__ feat) {
    __shared__ __attribute__((aligned(16))) CfSmem<E> sm;
    const int tid = threadIdx.x, lane = tid & 63, wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int h = lane >> 5, c = lane & 31;
    constexpr int TM = 32 * NW;
    for (int i = tid; i < CF_BIAS_ROWS * 256; i += 64 * NW) {
        const int row = i >> 8, r = i & 255;
        float v;
        if (row < 8) v = ba[net.s[row].bias + r] * SP_SCALE;
        else if (row == 8) v = r < 32 ? ba[net.shead.bias + r] * SP_SCALE : 0.f;
        else v = ba[net.sfeat.bias + r] * SP_SCALE;
        sm.bias[i] = v;
    }
    __syncthreads();
    const int ntiles = (n + TM - 1) / TM;
    if ((int)blockIdx.x >= ntiles) return;

    Pipe<E, NW, CF_STAGES> P;
    pipe_init(P, stream, sm, wave, lane, NW, CF_STAGES);

    for (int tile = blockIdx.x; tile < ntiles; tile += gridDim.x) {
        const int s = tile * TM + wave * 32 + c;
        const bool live = s < n;
        float cp[3] = {0.f, 0.f, 0.f};
        if (live) { cp[0] = cpts[3 * (size_t)s]; cp[1] = cpts[3 * (size_t)s + 1]; cp[2] = cpts[3 * (size_t)s + 2]; }
        EpiAux aux;
        aux.bits = 0u; aux.scale = SP_INV; aux.st = nullptr; aux.dbg = nullptr;
        unsigned* nobits = nullptr;
        P.template fetch<0>(); P.template fetch<1>(); P.template fetch<2>(); P.template fetch<3>();
        u32x4 B0[16], B1[16], Bp[4];
        f32x16 accA, accB;
        unsigned boff = 4 * h;                           // laundered as an integer: see mlp_fwd_tape_kernel
        asm volatile("" : "+v"(boff));
        const float* bias = sm.bias + boff;
        pe_frags_g<E, 8, true>(Bp, cp, h);
        fwd_layer<E, 4, EPI_SOFTPLUS, EPI_NONE, 0>(P, accA, accB, B0, Bp, B0, bias, h, aux, nobits);
        fwd_layer<E, 16, EPI_SOFTPLUS, EPI_SOFTPLUS, 0>(P, accA, accB, B0, Bp, B1, bias + 256, h, aux, nobits);
        fwd_layer<E, 16, EPI_SOFTPLUS, EPI_SOFTPLUS, 0>(P, accA, accB, B1, Bp, B0, bias + 512, h, aux, nobits);
        fwd_layer<E, 16, EPI_SOFTPLUS, EPI_SOFTPLUS, 0>(P, accA, accB, B0, Bp, B1, bias + 768, h, aux, nobits);
        fwd_layer<E, 20, EPI_SOFTPLUS, EPI_SOFTPLUS, 0>(P, accA, accB, B1, Bp, B0, bias + 1024, h, aux, nobits);
        fwd_layer<E, 16, EPI_SOFTPLUS, EPI_SOFTPLUS, 0>(P, accA, accB, B0, Bp, B1, bias + 1280, h, aux, nobits);
        fwd_layer<E, 16, EPI_SOFTPLUS, EPI_SOFTPLUS, 0>(P, accA, accB, B1, Bp, B0, bias + 1536, h, aux, nobits);
        fwd_layer<E, 16, EPI_SOFTPLUS, EPI_SOFTPLUS, 0>(P, accA, accB, B0, Bp, B1, bias + 1792, h, aux, nobits);
        // head row block: carries layer 7's pending epilogue into B1[14], B1[15]; the distance itself is not kept
        rbg<E, 0, 16, EPI_SOFTPLUS, true, false, true, 0, false>(P, accA, accB, B1, Bp, B1[14], B1[15], bias + 2048, h, aux);
        {   // feature rows: lin8 rows 1..256, no activation, rounded to the operand type as the heads read them
            const float* fb = bias + 2304;
            rbg<E, 0, 16, EPI_NONE, false, false, true, 0, false>(P, accB, accA, B1, Bp, B0[0], B0[1], fb, h, aux);
            rbg<E, 0, 16, EPI_LINEAR, false, false, true, 0, false>(P, accA, accB, B1, Bp, B0[0], B0[1], fb + 32, h, aux);
            rbg<E, 0, 16, EPI_LINEAR, false, false, true, 0, false>(P, accB, accA, B1, Bp, B0[2], B0[3], fb + 64, h, aux);
            rbg<E, 0, 16, EPI_LINEAR, false, false, true, 0, false>(P, accA, accB, B1, Bp, B0[4], B0[5], fb + 96, h, aux);
            rbg<E, 0, 16, EPI_LINEAR, false, false, true, 0, false>(P, accB, accA, B1, Bp, B0[6], B0[7], fb + 128, h, aux);
            rbg<E, 0, 16, EPI_LINEAR, false, false, true, 0, false>(P, accA, accB, B1, Bp, B0[8], B0[9], fb + 160, h, aux);
            rbg<E, 0, 16, EPI_LINEAR, false, false, true, 0, false>(P, accB, accA, B1, Bp, B0[10], B0[11], fb + 192, h, aux);
            rbg<E, 0, 16, EPI_LINEAR, false, true, true, 0, false>(P, accA, accB, B1, Bp, B0[12], B0[13], fb + 224, h, aux);
            flush<E, EPI_LINEAR, 0, false>(accA, B0[14], B0[15], h, aux);
        }
        if (live) {          // fragment k, element j of lane (c, h) is feature 32 (k / 2) + 16 (k % 2) + 8 (j / 4) + 4 h + j % 4
            float* o = feat + (size_t)s * 256 + 4 * h;
#pragma unroll
            for (int k = 0; k < 16; ++k)
#pragma unroll
                for (int j = 0; j < 8; ++j) {
                    const int f = 32 * (k >> 1) + 16 * (k & 1) + 8 * (j >> 2) + (j & 3);
                    o[f] = half_of<E>(B0[k][j >> 1], j & 1);
                }
        }
        asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    }
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    __builtin_amdgcn_s_barrier();
}

}  // namespace

template <typename E>
static void launch_canon_feat(const GeoNet& net, const void* fwd_arena, const float* barena, const float* cpts, int n, float* feat, hipStream_t stream) {
    if (n <= 0) return;
    constexpr int NW = RA_K4_NW_F;
    const int tiles = (n + 32 * NW - 1) / (32 * NW);
    const int grid = tiles < 256 ? tiles : 256;
    const char* sdf_half = reinterpret_cast<const char*>(fwd_arena) + (size_t)CF_SKIP_FRAGS * 1024;
    hipLaunchKernelGGL((sdf_feat_kernel<E, NW>), dim3(grid), dim3(64 * NW), 0, stream, net, (const void*)sdf_half, barena, cpts, n, feat);
}
