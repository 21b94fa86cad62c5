// LPIPS v0.1 with the VGG16 trunk (third_parties/lpips/lpips.py:23-124, pretrained_networks.py:96-134): forward and input
// gradient in exact fp32, for the perceptual term of the training objective (lossweights.lpips, trainer.py:92-106).
//
// Layout.  Activations are NHWC, so channels are the contiguous K dimension of every conv.  pred (in0) and target (in1) run
// as ONE batch of 2N images, so each conv layer is one launch and its weights stream once per pass.
//
// conv3x3 (pad 1, stride 1) is an implicit GEMM  out[M = B*H*W, Co] = im2col(in)[M, 9*C] x Wp[9*C, Co]  on
// v_mfma_f32_32x32x2_f32 (a k-ordered fmaf chain, no reduced precision).  Block tile 64 x 64, K step 32, 4 waves of 32 x 32;
// the next K step is prefetched into registers while the current one is multiplied out of LDS.  With C % 32 == 0 a K step
// lies inside one tap (ky, kx) and is 32 consecutive channels: two float4 loads per thread.  conv1_1 (C = 3, K = 27) takes
// the scalar operand path with K padded to 32 by zero weight rows.  Layers with few output tiles (conv3-conv5 at patch size)
// split K over blockIdx.z into partials that a second kernel sums in z order -- no float atomics, so every pass is bitwise
// deterministic.  The epilogue adds the bias and applies ReLU (forward) or the ReLU mask of the layer below (data gradient).
//
// The data gradient of a conv is the same GEMM over the rotated, transposed weights:
//   dx[b,y,x,ci] = sum_{ky,kx,co} g[b, y+ky-1, x+kx-1, co] * W[co, ci, 2-ky, 2-kx]
// packed once at load (occnerf_lpips_pack) next to the forward layout.  The trunk is frozen (trainer.py:69): no weight
// gradient.  Max-pools (2x2/2, floored) route the gradient to the first maximum of the window in row-major order, as torch's
// max_pool2d does; the head's gradient and the pool's are summed and masked by the tap's ReLU in one pass.
#include <algorithm>
#include <utility>

#include "common.h"

namespace occ {
namespace lp {

constexpr int kLayers = 13;
constexpr int kTaps = 5;
constexpr int kCin[kLayers] = {3, 64, 64, 128, 128, 256, 256, 256, 512, 512, 512, 512, 512};
constexpr int kCout[kLayers] = {64, 64, 128, 128, 256, 256, 256, 512, 512, 512, 512, 512, 512};
constexpr bool kPoolBefore[kLayers] = {false, false, true, false, true, false, false, true, false, false, true, false, false};
constexpr int kTapLayer[kTaps] = {1, 3, 6, 9, 12};        // relu1_2, relu2_2, relu3_3, relu4_3, relu5_3
constexpr float kEps = 1e-10f;                              // normalize_tensor, both places

constexpr int BM = 64, BN = 64, BK = 32, NT = 256;
constexpr int AP = BM + 4;                                  // LDS row pitch of the A tile (k-major)

inline int64_t round_up(int64_t a, int64_t b) { return (a + b - 1) / b * b; }

// Packed blob (floats), built by occnerf_lpips_pack: per layer the forward operand Wf[Kf][Nf] (Kf = round_up(9 Cin, 32),
// Nf = round_up(Cout, 64), k = (ky*3+kx)*Cin + ci), the data-gradient operand Wd[Kd][Nd] (Kd = 9 Cout,
// Nd = round_up(Cin, 64), k = (ky*3+kx)*Cout + co holding W[co, ci, 2-ky, 2-kx]) and the bias; then the five lin
// weights and the scaling layer's shift[3], scale[3].  Padding rows and columns are zero.
struct Pack {
    int64_t wf[kLayers], wd[kLayers], bias[kLayers], lin[kTaps], shift, scale, total;
    int kf[kLayers], nf[kLayers], kd[kLayers], nd[kLayers];
};

inline Pack pack_layout() {
    Pack p;
    int64_t o = 0;
    for (int l = 0; l < kLayers; l++) {
        p.kf[l] = (int)round_up(9 * kCin[l], BK);
        p.nf[l] = (int)round_up(kCout[l], BN);
        p.kd[l] = 9 * kCout[l];
        p.nd[l] = (int)round_up(kCin[l], BN);
        p.wf[l] = o;
        o += (int64_t)p.kf[l] * p.nf[l];
        p.wd[l] = o;
        o += (int64_t)p.kd[l] * p.nd[l];
        p.bias[l] = o;
        o += round_up(kCout[l], 4);
    }
    for (int t = 0; t < kTaps; t++) {
        p.lin[t] = o;
        o += kCout[kTapLayer[t]];
    }
    p.shift = o;
    o += 4;
    p.scale = o;
    o += 4;
    p.total = o;
    return p;
}

// Spatial size of each layer's input/output (same, pad 1) for an H x W image.
struct Geo {
    int h[kLayers], w[kLayers];
};
inline Geo geometry(int H, int W) {
    Geo g;
    int h = H, w = W;
    for (int l = 0; l < kLayers; l++) {
        if (kPoolBefore[l]) {
            h /= 2;
            w /= 2;
        }
        g.h[l] = h;
        g.w[l] = w;
    }
    return g;
}

// Split of K over blockIdx.z: enough blocks for two per CU, at least three K steps per split, at most 32 splits.
inline int splits_for(int64_t M, int N, int K) {
    const int64_t tiles = ((M + BM - 1) / BM) * ((N + BN - 1) / BN);
    const int ktiles = K / BK;
    int s = (int)std::max<int64_t>(1, (2 * kNumCU) / std::max<int64_t>(1, tiles));
    s = std::min(s, std::max(1, ktiles / 3));
    return std::min(s, 32);
}

// Workspace (floats), laid out by the host for a given (N, H, W); the forward fills it and the backward reads it.
struct Work {
    int64_t x, act[kLayers], pool[kTaps - 1], respix[kTaps], res, ga, gb, gh, part, total;
};
inline Work work_layout(int N, int H, int W) {
    const Geo g = geometry(H, W);
    const int64_t B = 2 * (int64_t)N;
    Work w;
    int64_t o = 0;
    auto take = [&](int64_t n) {
        const int64_t at = o;
        o += round_up(n, 64);
        return at;
    };
    w.x = take(B * H * W * 3);
    int64_t gmax = B * H * W * 3, part = 0;
    int pool = 0;
    for (int l = 0; l < kLayers; l++) {
        const int64_t n = B * g.h[l] * g.w[l] * kCout[l];
        w.act[l] = take(n);
        gmax = std::max(gmax, n);
        const int64_t M = B * g.h[l] * g.w[l];
        const int sf = splits_for(M, kCout[l], (int)round_up(9 * kCin[l], BK));
        if (sf > 1) part = std::max(part, sf * M * kCout[l]);
        for (int64_t Md : {M, M / 2}) {                     // the backward runs on one or both halves of the batch
            const int sd = splits_for(Md, kCin[l], 9 * kCout[l]);
            if (sd > 1) part = std::max(part, sd * Md * kCin[l]);
        }
        if (l + 1 < kLayers && kPoolBefore[l + 1]) w.pool[pool++] = take(B * g.h[l + 1] * g.w[l + 1] * kCout[l]);
    }
    for (int t = 0; t < kTaps; t++) {
        const int l = kTapLayer[t];
        w.respix[t] = take((int64_t)N * g.h[l] * g.w[l]);
    }
    w.res = take(kTaps * (int64_t)N);
    w.ga = take(gmax);
    w.gb = take(gmax);
    w.gh = take(gmax);
    w.part = take(std::max<int64_t>(part, 1));
    w.total = o;
    return w;
}

// ---------------------------------------------------------------------------------------------------------------------
// conv3x3 implicit GEMM

struct ConvArgs {
    const float *in;      // [B, H, W, C]
    const float *w;       // [Kp, Np]
    const float *bias;    // [Co] or null
    const float *mask;    // [B, H, W, Co] or null: out = mask > 0 ? out : 0
    float *out;           // [B, H, W, Co], or partials [splits, M, Co]
    int B, H, W, C, Co, Np, K, ktiles, splits, relu;
    int64_t M;
};

__device__ __forceinline__ float conv_epilogue(const ConvArgs &a, int64_t m, int n, float v) {
    if (a.bias) v = v + a.bias[n];
    if (a.relu) v = v > 0.0f ? v : 0.0f;
    if (a.mask && !(a.mask[m * a.Co + n] > 0.0f)) v = 0.0f;
    return v;
}

template <bool kSmallC>
__global__ __launch_bounds__(NT) void conv3x3_kernel(ConvArgs a) {
    __shared__ float As[BK * AP];
    __shared__ float Bs[BK * BN];
    const int t = threadIdx.x, lane = t & 63, wave = t >> 6;
    const int wm = wave & 1, wn = wave >> 1;
    const int64_t m0 = (int64_t)blockIdx.x * BM;
    const int n0 = blockIdx.y * BN;
    const int z = blockIdx.z;
    const int kt0 = (int)((int64_t)z * a.ktiles / a.splits), kt1 = (int)((int64_t)(z + 1) * a.ktiles / a.splits);

    // A loader: row r of the tile, 8 consecutive k at q*8
    const int ar = t >> 2, aq = t & 3;
    const int64_t am = m0 + ar;
    const bool arow = am < a.M;
    int ab = 0, ay = 0, ax = 0;
    if (arow) {
        const int64_t hw = (int64_t)a.H * a.W;
        ab = (int)(am / hw);
        const int rem = (int)(am - (int64_t)ab * hw);
        ay = rem / a.W;
        ax = rem - ay * a.W;
    }
    // B loader: k row t>>3, 8 consecutive columns at (t&7)*8
    const int br = t >> 3, bc = (t & 7) * 8;

    float ra[8], rb[8];
    auto load = [&](int kt) {
        const int k0 = kt * BK;
        if (kSmallC) {
#pragma unroll
            for (int j = 0; j < 8; j++) {
                const int k = k0 + aq * 8 + j;
                float v = 0.0f;
                if (arow && k < a.K) {
                    const int tap = k / a.C, ci = k - tap * a.C;
                    const int yy = ay + tap / 3 - 1, xx = ax + tap % 3 - 1;
                    if (yy >= 0 && yy < a.H && xx >= 0 && xx < a.W)
                        v = a.in[(((int64_t)ab * a.H + yy) * a.W + xx) * a.C + ci];
                }
                ra[j] = v;
            }
        } else {
            const int tap = k0 / a.C, ci0 = k0 - tap * a.C;
            const int yy = ay + tap / 3 - 1, xx = ax + tap % 3 - 1;
            if (arow && yy >= 0 && yy < a.H && xx >= 0 && xx < a.W) {
                const float4 *src =
                    reinterpret_cast<const float4 *>(a.in + (((int64_t)ab * a.H + yy) * a.W + xx) * a.C + ci0 + aq * 8);
                const float4 v0 = src[0], v1 = src[1];
                ra[0] = v0.x; ra[1] = v0.y; ra[2] = v0.z; ra[3] = v0.w;
                ra[4] = v1.x; ra[5] = v1.y; ra[6] = v1.z; ra[7] = v1.w;
            } else {
#pragma unroll
                for (int j = 0; j < 8; j++) ra[j] = 0.0f;
            }
        }
        const float4 *wsrc = reinterpret_cast<const float4 *>(a.w + (int64_t)(k0 + br) * a.Np + n0 + bc);
        const float4 w0 = wsrc[0], w1 = wsrc[1];
        rb[0] = w0.x; rb[1] = w0.y; rb[2] = w0.z; rb[3] = w0.w;
        rb[4] = w1.x; rb[5] = w1.y; rb[6] = w1.z; rb[7] = w1.w;
    };

    using f32x16 = __attribute__((ext_vector_type(16))) float;
    f32x16 acc;
#pragma unroll
    for (int i = 0; i < 16; i++) acc[i] = 0.0f;

    if (kt0 < kt1) load(kt0);
    for (int kt = kt0; kt < kt1; kt++) {
        __syncthreads();
#pragma unroll
        for (int j = 0; j < 8; j++) As[(aq * 8 + j) * AP + ar] = ra[j];
        *reinterpret_cast<float4 *>(&Bs[br * BN + bc]) = make_float4(rb[0], rb[1], rb[2], rb[3]);
        *reinterpret_cast<float4 *>(&Bs[br * BN + bc + 4]) = make_float4(rb[4], rb[5], rb[6], rb[7]);
        __syncthreads();
        if (kt + 1 < kt1) load(kt + 1);
        const int kl = lane >> 5, il = lane & 31;
#pragma unroll
        for (int kk = 0; kk < BK; kk += 2) {
            const float av = As[(kk + kl) * AP + wm * 32 + il];
            const float bv = Bs[(kk + kl) * BN + wn * 32 + il];
            acc = __builtin_amdgcn_mfma_f32_32x32x2f32(av, bv, acc, 0, 0, 0);
        }
    }

    // C/D map of 32x32: col = lane & 31, row = (i & 3) + 8 (i >> 2) + 4 (lane >> 5)
    const int n = n0 + wn * 32 + (lane & 31);
    if (n >= a.Co) return;
#pragma unroll
    for (int i = 0; i < 16; i++) {
        const int64_t m = m0 + wm * 32 + (i & 3) + 8 * (i >> 2) + 4 * (lane >> 5);
        if (m >= a.M) continue;
        if (a.splits == 1) a.out[m * a.Co + n] = conv_epilogue(a, m, n, acc[i]);
        else a.out[((int64_t)z * a.M + m) * a.Co + n] = acc[i];
    }
}

// Sum of the split-K partials in z order, then the epilogue.
__global__ __launch_bounds__(256) void conv_reduce_kernel(ConvArgs a, const float *__restrict__ part, float *__restrict__ out) {
    const int64_t e = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    const int64_t total = a.M * a.Co;
    if (e >= total) return;
    float v = part[e];
    for (int z = 1; z < a.splits; z++) v += part[(int64_t)z * total + e];
    out[e] = conv_epilogue(a, e / a.Co, (int)(e % a.Co), v);
}

// in[B,H,W,C] (x) wpk[Kp,Np] -> out[B,H,W,Co]
int conv3x3(const float *in, int B, int H, int W, int C, int Co, const float *wpk, int Np, const float *bias, int relu,
            const float *mask, float *out, float *part, hipStream_t s) {
    ConvArgs a;
    a.in = in;
    a.w = wpk;
    a.bias = bias;
    a.mask = mask;
    a.B = B;
    a.H = H;
    a.W = W;
    a.C = C;
    a.Co = Co;
    a.Np = Np;
    a.K = 9 * C;
    a.ktiles = (int)(round_up(a.K, BK) / BK);
    a.relu = relu;
    a.M = (int64_t)B * H * W;
    a.splits = splits_for(a.M, Co, (int)round_up(a.K, BK));
    a.out = a.splits > 1 ? part : out;
    const dim3 grid((unsigned)((a.M + BM - 1) / BM), (unsigned)((Co + BN - 1) / BN), (unsigned)a.splits);
    if (C % BK == 0) hipLaunchKernelGGL(conv3x3_kernel<false>, grid, dim3(NT), 0, s, a);
    else hipLaunchKernelGGL(conv3x3_kernel<true>, grid, dim3(NT), 0, s, a);
    if (a.splits > 1) {
        const int64_t n = a.M * Co;
        hipLaunchKernelGGL(conv_reduce_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, s, a, part, out);
    }
    return check_launch("lpips conv3x3");
}

// ---------------------------------------------------------------------------------------------------------------------
// elementwise passes

// (x - shift) / scale of in0 (images 0..N-1) and in1 (N..2N-1), NCHW or NHWC, into x[2N,H,W,3]
__global__ __launch_bounds__(256) void scale_in_kernel(const float *__restrict__ in0, const float *__restrict__ in1, int N,
                                                       int H, int W, int nhwc, const float *__restrict__ shift,
                                                       const float *__restrict__ scale, float *__restrict__ x) {
    const int64_t e = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    const int64_t hw = (int64_t)H * W, per = hw * 3;
    if (e >= 2 * N * per) return;
    const int b = (int)(e / per);
    const int64_t r = e - b * per;              // NHWC offset inside the image
    const int c = (int)(r % 3);
    const int64_t p = r / 3;
    const float *src = b < N ? in0 + (int64_t)b * per : in1 + (int64_t)(b - N) * per;
    const float v = nhwc ? src[r] : src[c * hw + p];
    x[e] = (v - shift[c]) / scale[c];
}

// d in = dx / scale, back to the caller's layout, for images [b0, b0 + nb) of the batch; dx indexed from b0
__global__ __launch_bounds__(256) void scale_out_kernel(const float *__restrict__ dx, int N, int b0, int nb, int H, int W,
                                                        int nhwc, const float *__restrict__ scale, float *__restrict__ d0,
                                                        float *__restrict__ d1) {
    const int64_t e = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    const int64_t hw = (int64_t)H * W, per = hw * 3;
    if (e >= (int64_t)nb * per) return;
    const int b = b0 + (int)(e / per);
    const int64_t r = e % per;
    const int c = (int)(r % 3);
    const int64_t p = r / 3;
    float *dst = b < N ? d0 + (int64_t)b * per : d1 + (int64_t)(b - N) * per;
    dst[nhwc ? r : c * hw + p] = dx[e] / scale[c];
}

// 2x2/2 max-pool, floored: in[B,h,w,C] -> out[B,h/2,w/2,C]
__global__ __launch_bounds__(256) void maxpool_kernel(const float *__restrict__ in, int B, int h, int w, int C,
                                                      float *__restrict__ out) {
    const int h2 = h / 2, w2 = w / 2;
    const int64_t e = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (e >= (int64_t)B * h2 * w2 * C) return;
    const int c = (int)(e % C);
    int64_t p = e / C;
    const int x2 = (int)(p % w2);
    p /= w2;
    const int y2 = (int)(p % h2);
    const int b = (int)(p / h2);
    const float *s = in + (((int64_t)b * h + 2 * y2) * w + 2 * x2) * C + c;
    float m = s[0];
    const float v1 = s[C], v2 = s[(int64_t)w * C], v3 = s[(int64_t)w * C + C];
    if (v1 > m) m = v1;
    if (v2 > m) m = v2;
    if (v3 > m) m = v3;
    out[e] = m;
}

// Gradient at a tap's relu output: (act > 0) * (ghead + the pool's gradient if this element is the first maximum of its
// window).  act, ghead, out [nb,h,w,C]; gpool [nb,h/2,w/2,C] (all offset to the first image of the range).
__global__ __launch_bounds__(256) void pool_back_kernel(const float *__restrict__ act, const float *__restrict__ ghead,
                                                        const float *__restrict__ gpool, int nb, int h, int w, int C,
                                                        float *__restrict__ out) {
    const int64_t e = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (e >= (int64_t)nb * h * w * C) return;
    const float a = act[e];
    if (!(a > 0.0f)) {
        out[e] = 0.0f;
        return;
    }
    float v = ghead[e];
    const int c = (int)(e % C);
    int64_t p = e / C;
    const int x = (int)(p % w);
    p /= w;
    const int y = (int)(p % h);
    const int b = (int)(p / h);
    const int h2 = h / 2, w2 = w / 2, y2 = y >> 1, x2 = x >> 1;
    if (y2 < h2 && x2 < w2) {
        const float *s = act + (((int64_t)b * h + 2 * y2) * w + 2 * x2) * C + c;
        const float q[4] = {s[0], s[C], s[(int64_t)w * C], s[(int64_t)w * C + C]};
        int arg = 0;
        float m = q[0];
#pragma unroll
        for (int i = 1; i < 4; i++)
            if (q[i] > m) {
                m = q[i];
                arg = i;
            }
        if (arg == (y - 2 * y2) * 2 + (x - 2 * x2)) v = v + gpool[(((int64_t)b * h2 + y2) * w2 + x2) * C + c];
    }
    out[e] = v;
}

// ---------------------------------------------------------------------------------------------------------------------
// LPIPS head: one wave per pixel of an image pair, channels over the lanes (C <= 512: up to 8 per lane)

__device__ __forceinline__ float wave_sum(float v) {
#pragma unroll
    for (int o = 32; o >= 1; o >>= 1) v += __shfl_xor(v, o);
    return v;
}

// respix[n, p] = sum_c lin[c] (f0/(|f0|+eps) - f1/(|f1|+eps))^2 with f0 = act[n], f1 = act[N + n]
__global__ __launch_bounds__(256) void head_fwd_kernel(const float *__restrict__ act, int N, int hw, int C,
                                                       const float *__restrict__ lin, float *__restrict__ respix) {
    const int lane = threadIdx.x & 63;
    const int64_t pix = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
    if (pix >= (int64_t)N * hw) return;
    const int n = (int)(pix / hw);
    const int64_t p = pix - (int64_t)n * hw;
    const float *f0 = act + ((int64_t)n * hw + p) * C;
    const float *f1 = act + ((int64_t)(N + n) * hw + p) * C;
    const int J = C >> 6;
    float a[8], b[8], s0 = 0.0f, s1 = 0.0f;
#pragma unroll
    for (int j = 0; j < 8; j++)
        if (j < J) {
            a[j] = f0[j * 64 + lane];
            b[j] = f1[j * 64 + lane];
            s0 = __fmaf_rn(a[j], a[j], s0);
            s1 = __fmaf_rn(b[j], b[j], s1);
        }
    const float d0 = sqrtf(wave_sum(s0) + kEps) + kEps, d1 = sqrtf(wave_sum(s1) + kEps) + kEps;
    float r = 0.0f;
#pragma unroll
    for (int j = 0; j < 8; j++)
        if (j < J) {
            const float d = a[j] / d0 - b[j] / d1;
            r = __fmaf_rn(lin[j * 64 + lane], d * d, r);
        }
    r = wave_sum(r);
    if (lane == 0) respix[pix] = r;
}

// res[t, n] = mean_p respix_t[n, p]; val[n] = res[0, n] + ... + res[4, n].  One block per image, fixed reduction order.
struct HeadSizes {
    int hw[kTaps];
    const float *respix[kTaps];
};
__global__ __launch_bounds__(256) void head_finish_kernel(HeadSizes hs, int N, float *__restrict__ res,
                                                          float *__restrict__ val) {
    __shared__ float red[256];
    const int n = blockIdx.x, t = threadIdx.x;
    float v = 0.0f;
    for (int k = 0; k < kTaps; k++) {
        const int hw = hs.hw[k];
        const float *src = hs.respix[k] + (int64_t)n * hw;
        float s = 0.0f;
        for (int i = t; i < hw; i += 256) s += src[i];
        red[t] = s;
        __syncthreads();
        for (int o = 128; o > 0; o >>= 1) {
            if (t < o) red[t] += red[t + o];
            __syncthreads();
        }
        const float r = red[0] / (float)hw;
        __syncthreads();
        v = k == 0 ? r : v + r;
        if (t == 0 && res) res[k * N + n] = r;
    }
    if (t == 0) val[n] = v;
}

// d act for in0 (need0) / in1 (need1) of one tap given gres[n] = d loss / d res_t[n], masked by act > 0.
__global__ __launch_bounds__(256) void head_bwd_kernel(const float *__restrict__ act, int N, int hw, int C,
                                                       const float *__restrict__ lin, const float *__restrict__ gres,
                                                       int need0, int need1, float *__restrict__ g) {
    const int lane = threadIdx.x & 63;
    const int64_t pix = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
    if (pix >= (int64_t)N * hw) return;
    const int n = (int)(pix / hw);
    const int64_t p = pix - (int64_t)n * hw;
    const int64_t o0 = ((int64_t)n * hw + p) * C, o1 = ((int64_t)(N + n) * hw + p) * C;
    const int J = C >> 6;
    float a[8], b[8], s0 = 0.0f, s1 = 0.0f;
#pragma unroll
    for (int j = 0; j < 8; j++)
        if (j < J) {
            a[j] = act[o0 + j * 64 + lane];
            b[j] = act[o1 + j * 64 + lane];
            s0 = __fmaf_rn(a[j], a[j], s0);
            s1 = __fmaf_rn(b[j], b[j], s1);
        }
    const float n0 = sqrtf(wave_sum(s0) + kEps), n1 = sqrtf(wave_sum(s1) + kEps);
    const float d0 = n0 + kEps, d1 = n1 + kEps;
    const float coef = gres[n] / (float)hw;                 // mean over pixels
    float u[8], dot0 = 0.0f, dot1 = 0.0f;
#pragma unroll
    for (int j = 0; j < 8; j++)
        if (j < J) {
            const float d = a[j] / d0 - b[j] / d1;
            u[j] = coef * lin[j * 64 + lane] * 2.0f * d;    // d loss / d (f0 normalised); the f1 side is -u
            dot0 = __fmaf_rn(u[j], a[j], dot0);
            dot1 = __fmaf_rn(u[j], b[j], dot1);
        }
    // f / d with d = sqrt(|f|^2 + eps) + eps:  df_j = u_j / d - (sum_c u_c f_c) f_j / (d^2 |f|)
    const float k0 = wave_sum(dot0) / (d0 * d0 * n0), k1 = wave_sum(dot1) / (d1 * d1 * n1);
#pragma unroll
    for (int j = 0; j < 8; j++)
        if (j < J) {
            const int c = j * 64 + lane;
            if (need0) g[o0 + c] = a[j] > 0.0f ? u[j] / d0 - k0 * a[j] : 0.0f;
            if (need1) g[o1 + c] = b[j] > 0.0f ? -u[j] / d1 + k1 * b[j] : 0.0f;
        }
}

// ---------------------------------------------------------------------------------------------------------------------
// weight pack

struct PackSrc {
    const float *lin[kTaps];
    const float *shift, *scale;
};

__global__ __launch_bounds__(256) void pack_layer_kernel(const float *__restrict__ w, const float *__restrict__ bias, int Cin,
                                                         int Cout, int kf, int nf, int kd, int nd, float *__restrict__ wf,
                                                         float *__restrict__ wd, float *__restrict__ bo) {
    const int64_t e = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    const int64_t nF = (int64_t)kf * nf, nD = (int64_t)kd * nd;
    if (e < nF) {
        const int k = (int)(e / nf), co = (int)(e % nf);
        float v = 0.0f;
        if (k < 9 * Cin && co < Cout) {
            const int tap = k / Cin, ci = k % Cin;
            v = w[((int64_t)co * Cin + ci) * 9 + tap];
        }
        wf[e] = v;
    } else if (e < nF + nD) {
        const int64_t f = e - nF;
        const int k = (int)(f / nd), ci = (int)(f % nd);
        float v = 0.0f;
        if (ci < Cin) {
            const int tap = k / Cout, co = k % Cout;
            v = w[((int64_t)co * Cin + ci) * 9 + (8 - tap)];       // W[co, ci, 2-ky, 2-kx]
        }
        wd[f] = v;
    } else if (e < nF + nD + Cout) {
        bo[e - nF - nD] = bias[e - nF - nD];
    }
}

__global__ void pack_small_kernel(PackSrc src, float *__restrict__ lin, float *__restrict__ shift, float *__restrict__ scale,
                                  int64_t lin_stride0, int64_t lin_stride1, int64_t lin_stride2, int64_t lin_stride3) {
    const int64_t off[kTaps + 1] = {0, lin_stride0, lin_stride1, lin_stride2, lin_stride3, 0};
    for (int t = 0; t < kTaps; t++) {
        const int C = kCout[kTapLayer[t]];
        for (int c = threadIdx.x; c < C; c += blockDim.x) lin[off[t] + c] = src.lin[t][c];
    }
    if (threadIdx.x < 3) {
        shift[threadIdx.x] = src.shift[threadIdx.x];
        scale[threadIdx.x] = src.scale[threadIdx.x];
    }
}

}  // namespace lp
}  // namespace occ

using namespace occ;
using namespace occ::lp;

OCC_API int64_t occnerf_lpips_packed_floats(void) { return pack_layout().total; }

OCC_API int64_t occnerf_lpips_workspace_floats(int32_t N, int32_t H, int32_t W) {
    if (N < 1 || H < 16 || W < 16) return -1;
    return work_layout(N, H, W).total;
}

OCC_API int occnerf_lpips_pack(const float *const *h_conv_w, const float *const *h_conv_b, const float *const *h_lin,
                               const float *shift, const float *scale, float *packed, void *stream) {
    OCC_REQUIRE(h_conv_w && h_conv_b && h_lin && shift && scale && packed, "lpips_pack: null argument");
    for (int l = 0; l < kLayers; l++)
        OCC_REQUIRE(h_conv_w[l] && h_conv_b[l], "lpips_pack: null weight or bias of conv layer %d", l);
    for (int t = 0; t < kTaps; t++) OCC_REQUIRE(h_lin[t], "lpips_pack: null lin weight %d", t);
    const Pack p = pack_layout();
    hipStream_t s = as_stream(stream);
    for (int l = 0; l < kLayers; l++) {
        const int64_t n = (int64_t)p.kf[l] * p.nf[l] + (int64_t)p.kd[l] * p.nd[l] + kCout[l];
        hipLaunchKernelGGL(pack_layer_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, s, h_conv_w[l], h_conv_b[l],
                           kCin[l], kCout[l], p.kf[l], p.nf[l], p.kd[l], p.nd[l], packed + p.wf[l], packed + p.wd[l],
                           packed + p.bias[l]);
    }
    PackSrc src;
    for (int t = 0; t < kTaps; t++) src.lin[t] = h_lin[t];
    src.shift = shift;
    src.scale = scale;
    hipLaunchKernelGGL(pack_small_kernel, dim3(1), dim3(256), 0, s, src, packed + p.lin[0], packed + p.shift,
                       packed + p.scale, p.lin[1] - p.lin[0], p.lin[2] - p.lin[0], p.lin[3] - p.lin[0],
                       p.lin[4] - p.lin[0]);
    return check_launch("lpips_pack");
}

static int lpips_args(const char *what, const float *packed, float *work, int32_t N, int32_t H, int32_t W) {
    OCC_REQUIRE(N >= 1, "%s: N must be >= 1 (got %d)", what, N);
    OCC_REQUIRE(H >= 16 && W >= 16, "%s: H and W must be >= 16 so that relu5_3 is not empty (got %d x %d)", what, H, W);
    OCC_REQUIRE(packed && work, "%s: null packed weights or workspace", what);
    return 0;
}

OCC_API int occnerf_lpips_forward(const float *packed, const float *in0, const float *in1, int32_t N, int32_t H, int32_t W,
                                  int32_t in_nhwc, float *work, float *val, float *res, void *stream) {
    if (int rc = lpips_args("lpips_forward", packed, work, N, H, W)) return rc;
    OCC_REQUIRE(in0 && in1 && val, "lpips_forward: null in0, in1 or val");
    const Pack p = pack_layout();
    const Work w = work_layout(N, H, W);
    const Geo g = geometry(H, W);
    hipStream_t s = as_stream(stream);
    const int B = 2 * N;
    {
        const int64_t n = (int64_t)B * H * W * 3;
        hipLaunchKernelGGL(scale_in_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, s, in0, in1, N, H, W,
                           in_nhwc ? 1 : 0, packed + p.shift, packed + p.scale, work + w.x);
    }
    const float *x = work + w.x;
    int pool = 0;
    for (int l = 0; l < kLayers; l++) {
        if (kPoolBefore[l]) {
            const int hp = g.h[l - 1], wp = g.w[l - 1], C = kCin[l];
            const int64_t n = (int64_t)B * (hp / 2) * (wp / 2) * C;
            hipLaunchKernelGGL(maxpool_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, s, x, B, hp, wp, C,
                               work + w.pool[pool]);
            x = work + w.pool[pool++];
        }
        if (int rc = conv3x3(x, B, g.h[l], g.w[l], kCin[l], kCout[l], packed + p.wf[l], p.nf[l], packed + p.bias[l], 1,
                             nullptr, work + w.act[l], work + w.part, s))
            return rc;
        x = work + w.act[l];
    }
    HeadSizes hs;
    for (int t = 0; t < kTaps; t++) {
        const int l = kTapLayer[t], hw = g.h[l] * g.w[l];
        hs.hw[t] = hw;
        hs.respix[t] = work + w.respix[t];
        const int64_t pix = (int64_t)N * hw;
        hipLaunchKernelGGL(head_fwd_kernel, dim3((unsigned)((pix + 3) / 4)), dim3(256), 0, s, work + w.act[l], N, hw,
                           kCout[l], packed + p.lin[t], work + w.respix[t]);
    }
    hipLaunchKernelGGL(head_finish_kernel, dim3(N), dim3(256), 0, s, hs, N, res ? res : work + w.res, val);
    return check_launch("lpips_forward");
}

OCC_API int occnerf_lpips_backward(const float *packed, float *work, int32_t N, int32_t H, int32_t W, int32_t in_nhwc,
                                   const float *gres, float *d_in0, float *d_in1, void *stream) {
    if (int rc = lpips_args("lpips_backward", packed, work, N, H, W)) return rc;
    OCC_REQUIRE(gres, "lpips_backward: null gres");
    OCC_REQUIRE(d_in0 || d_in1, "lpips_backward: null d_in0 and d_in1 (nothing to compute)");
    const Pack p = pack_layout();
    const Work w = work_layout(N, H, W);
    const Geo g = geometry(H, W);
    hipStream_t s = as_stream(stream);
    const int need0 = d_in0 ? 1 : 0, need1 = d_in1 ? 1 : 0;
    const int b0 = need0 ? 0 : N, nb = (need0 + need1) * N;     // the images whose gradient is wanted
    auto at = [&](int64_t base, int l) { return work + base + (int64_t)b0 * g.h[l] * g.w[l] * kCout[l]; };
    float *ga = work + w.ga, *gb = work + w.gb, *gh = work + w.gh;
    // head gradient of tap t into buf (masked by the tap's relu), images indexed from 0 (the full batch)
    auto head = [&](int t, float *buf) {
        const int l = kTapLayer[t], hw = g.h[l] * g.w[l];
        const int64_t pix = (int64_t)N * hw;
        hipLaunchKernelGGL(head_bwd_kernel, dim3((unsigned)((pix + 3) / 4)), dim3(256), 0, s, work + w.act[l], N, hw,
                           kCout[l], packed + p.lin[t], gres + (int64_t)t * N, need0, need1, buf);
    };
    head(kTaps - 1, ga);                                    // d relu5_3
    int tap = kTaps - 2, pool = kTaps - 2;
    for (int l = kLayers - 1; l >= 0; l--) {
        // ga: gradient wrt act[l] (masked), full-batch indexing -> gradient wrt this conv's input into gb
        const int h = g.h[l], wd = g.w[l];
        const int64_t off_in = (int64_t)b0 * h * wd * kCout[l], off_out = (int64_t)b0 * h * wd * kCin[l];
        const float *mask = (l > 0 && !kPoolBefore[l]) ? at(w.act[l - 1], l - 1) : nullptr;
        if (int rc = conv3x3(ga + off_in, nb, h, wd, kCout[l], kCin[l], packed + p.wd[l], p.nd[l], nullptr, 0, mask,
                             gb + off_out, work + w.part, s))
            return rc;
        if (l == 0) break;
        if (kPoolBefore[l]) {
            // gb: gradient wrt pool output; combine with the head gradient of the tap below into ga
            head(tap, gh);
            const int lt = l - 1, ht = g.h[lt], wt = g.w[lt], C = kCout[lt];
            const int64_t n = (int64_t)nb * ht * wt * C;
            hipLaunchKernelGGL(pool_back_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, s, at(w.act[lt], lt),
                               gh + (int64_t)b0 * ht * wt * C, gb + (int64_t)b0 * (ht / 2) * (wt / 2) * C, nb, ht, wt, C,
                               ga + (int64_t)b0 * ht * wt * C);
            tap--;
            pool--;
        } else {
            std::swap(ga, gb);
        }
    }
    (void)pool;
    const int64_t n = (int64_t)nb * H * W * 3;
    hipLaunchKernelGGL(scale_out_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, s, gb + (int64_t)b0 * H * W * 3, N,
                       b0, nb, H, W, in_nhwc ? 1 : 0, packed + p.scale, d_in0, d_in1);
    return check_launch("lpips_backward");
}

// ---------------------------------------------------------------------------------------------------------------------
// patch images of the training batch (trainer.py:31-41 _unpack_imgs)

__global__ __launch_bounds__(256) void patch_assemble_kernel(const float *__restrict__ rgb, const int32_t *__restrict__ row_of_pix,
                                                             int64_t n_pix, float bg0, float bg1, float bg2,
                                                             float *__restrict__ img) {
    const int64_t e = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (e >= n_pix * 3) return;
    const int64_t p = e / 3;
    const int c = (int)(e - p * 3);
    const int32_t r = row_of_pix[p];
    img[e] = r >= 0 ? rgb[(int64_t)r * 3 + c] : (c == 0 ? bg0 : (c == 1 ? bg1 : bg2));
}

__global__ __launch_bounds__(256) void patch_assemble_back_kernel(const float *__restrict__ d_img,
                                                                  const int32_t *__restrict__ pix_of_row, int64_t R,
                                                                  float *__restrict__ d_rgb) {
    const int64_t e = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (e >= R * 3) return;
    const int64_t r = e / 3;
    d_rgb[e] = d_img[(int64_t)pix_of_row[r] * 3 + (e - r * 3)];
}

OCC_API int occnerf_patch_assemble(const float *rgb, const int32_t *row_of_pix, int64_t R, int32_t n_patches, int32_t size,
                                   const float *h_bgcolor01, float *img, void *stream) {
    OCC_REQUIRE(n_patches >= 1 && size >= 1 && R >= 0 && R <= (int64_t)n_patches * size * size,
                "patch_assemble: bad sizes (R %lld, %d patches of %d)", (long long)R, n_patches, size);
    OCC_REQUIRE(row_of_pix && h_bgcolor01 && img && (R == 0 || rgb), "patch_assemble: null argument");
    const int64_t n = (int64_t)n_patches * size * size;
    hipLaunchKernelGGL(patch_assemble_kernel, dim3((unsigned)((n * 3 + 255) / 256)), dim3(256), 0, as_stream(stream), rgb,
                       row_of_pix, n, h_bgcolor01[0], h_bgcolor01[1], h_bgcolor01[2], img);
    return check_launch("patch_assemble");
}

OCC_API int occnerf_patch_assemble_backward(const float *d_img, const int32_t *pix_of_row, int64_t R, float *d_rgb,
                                            void *stream) {
    OCC_REQUIRE(R >= 0, "patch_assemble_backward: bad R");
    OCC_REQUIRE(R == 0 || (d_img && pix_of_row && d_rgb), "patch_assemble_backward: null argument");
    if (R == 0) return 0;
    hipLaunchKernelGGL(patch_assemble_back_kernel, dim3((unsigned)((R * 3 + 255) / 256)), dim3(256), 0, as_stream(stream),
                       d_img, pix_of_row, R, d_rgb);
    return check_launch("patch_assemble_backward");
}
