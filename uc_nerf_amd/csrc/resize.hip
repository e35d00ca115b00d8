// f4, Pillow's Image.resize(img_wh, BILINEAR) of the colour frames (data/scared.py:450-451, data/hamlyn.py:507-508, data/finetune.py:445-446) on the
// device, bit for bit: ImagingResample for 8-bit channels.  For a down-scale that is an antialiased triangle filter in fixed point: per axis a
// table of (start, count, 22-bit integer coefficients) per output pixel, a horizontal pass whose result is rounded and clipped to BYTES, then a
// vertical pass on those bytes.  The tables are host arithmetic in double (ucnerf_resize_bilinear_coeffs below; the build's -ffp-contract=off keeps
// every multiply and add separate); the device does integer arithmetic only.  Plain HIP C++, wave64, plain vector stores, no atomics.
//
// ONE launch for N frames, both passes.  A workgroup (256 threads) owns RS_TY x RS_TX output pixels of one frame (blockIdx.z):
//   tables     the tile's starts, counts and coefficients go to LDS, every start and count clamped into what the tile stages (so that tables other
//              than the host function's cannot make a read leave src)
//   stage-in   the input rows y0 .. y1 the tile's vertical taps span, the columns its horizontal taps span, RAW_ROWS rows at a time: a wave reads
//              64 consecutive whole dwords of a row segment per instruction, four row pieces in flight per lane (the array's last, partial dword
//              byte by byte).  A row's first byte sits at offset (address & 3) of its LDS row.
//   horizontal one thread per (input row, output column) of the chunk, three channels: out of the raw LDS rows into the intermediate tile
//              [y1 - y0][RS_TX x 3] of BYTES -- rounded and clipped exactly as Pillow's, never kept wider
//   vertical   one thread per dword of an output row segment (its four bytes; the bytes of a dword that lie outside the tile are left alone: the
//              thread then stores bytes), out of the intermediate tile into dst.  A pad byte between 3 H W and the frame stride is never written.
// A pass along an axis of unchanged size is a copy (one tap, no arithmetic).
// LDS: up to 32 KB where the whole row span fits in it, never above 64 KB (the ratio bound UCNERF_RESIZE_MAX_RATIO is what guarantees that).
// Bound: the HBM read of the native frames.
#include "common.h"

#include <cmath>

namespace ucnerf {

constexpr int RS_BLOCK = 256;
constexpr int RS_WAVES = RS_BLOCK / 64;
constexpr int RS_TX = 32, RS_TY = 8;                         // output tile
constexpr int RS_MID_ROW = RS_TX * 3;                        // bytes of an intermediate row (a multiple of 4)
constexpr int RS_OUT_DW = RS_MID_ROW / 4 + 1;                // dwords an output row segment can touch
constexpr int RS_STAGE = 4;                                  // row pieces in flight per lane
constexpr int RS_LDS_TARGET = 32 * 1024, RS_LDS_MAX = 64 * 1024;
constexpr int RS_PRECISION = 22;
constexpr int RS_MAX_SIZE = 32768;

struct ResizeGeom {
    int seg_cols_cap;   // input columns a tile's horizontal taps can span
    int seg_dw_cap;     // dwords of a raw LDS row
    int mid_rows_cap;   // input rows a tile's vertical taps can span
    int raw_rows;       // rows staged at a time
};

__device__ __forceinline__ int rs_clamp(int v, int lo, int hi) { return v < lo ? lo : (v > hi ? hi : v); }
__device__ __forceinline__ int rs_clip8(int acc) { return rs_clamp(acc >> RS_PRECISION, 0, 255); }

__global__ void __launch_bounds__(RS_BLOCK) resize_bilinear_u8_kernel(ucnerf_resize_params p, ResizeGeom g) {
    extern __shared__ uint32_t rs_lds[];
    int* kxs = reinterpret_cast<int*>(rs_lds);               // [RS_TX][ksize_x]
    int* kys = kxs + RS_TX * p.ksize_x;                      // [RS_TY][ksize_y]
    int* sxs = kys + RS_TY * p.ksize_y;                      // start - seg_lo, count per tile column
    int* cxs = sxs + RS_TX;
    int* sys = cxs + RS_TX;                                  // start - y0, count per tile row
    int* cys = sys + RS_TY;
    uint8_t* mid = reinterpret_cast<uint8_t*>(cys + RS_TY);  // [mid_rows_cap][RS_MID_ROW]
    uint32_t* raw = reinterpret_cast<uint32_t*>(mid) + g.mid_rows_cap * (RS_MID_ROW / 4);   // [raw_rows][seg_dw_cap]

    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int f = blockIdx.z;
    const int ox0 = blockIdx.x * RS_TX, oy0 = blockIdx.y * RS_TY;
    const int tw = min(RS_TX, p.W - ox0), th = min(RS_TY, p.H - oy0);
    const bool hcopy = p.Win == p.W, vcopy = p.Hin == p.H;

    // what the tile reads: input columns seg_lo .. seg_hi, input rows y0 .. y1 (uniform)
    int seg_lo, seg_hi, y0, y1;
    if (hcopy) {
        seg_lo = ox0, seg_hi = ox0 + tw;
    } else {
        const int last = ox0 + tw - 1;
        seg_lo = rs_clamp(p.start_x[ox0], 0, p.Win);
        seg_hi = min(rs_clamp(p.start_x[last], seg_lo, p.Win) + rs_clamp(p.count_x[last], 0, p.ksize_x), min(p.Win, seg_lo + g.seg_cols_cap));
    }
    if (vcopy) {
        y0 = oy0, y1 = oy0 + th;
    } else {
        const int last = oy0 + th - 1;
        y0 = rs_clamp(p.start_y[oy0], 0, p.Hin);
        y1 = min(rs_clamp(p.start_y[last], y0, p.Hin) + rs_clamp(p.count_y[last], 0, p.ksize_y), min(p.Hin, y0 + g.mid_rows_cap));
    }
    for (int t = tid; t < tw; t += RS_BLOCK) {
        const int s = hcopy ? ox0 + t : rs_clamp(p.start_x[ox0 + t], seg_lo, seg_hi);
        sxs[t] = s - seg_lo;
        cxs[t] = hcopy ? 1 : min(rs_clamp(p.count_x[ox0 + t], 0, p.ksize_x), seg_hi - s);
    }
    for (int t = tid; t < th; t += RS_BLOCK) {
        const int s = vcopy ? oy0 + t : rs_clamp(p.start_y[oy0 + t], y0, y1);
        sys[t] = s - y0;
        cys[t] = vcopy ? 1 : min(rs_clamp(p.count_y[oy0 + t], 0, p.ksize_y), y1 - s);
    }
    if (!hcopy)
        for (int i = tid; i < tw * p.ksize_x; i += RS_BLOCK) kxs[i] = p.k_x[(long long)ox0 * p.ksize_x + i];
    if (!vcopy)
        for (int i = tid; i < th * p.ksize_y; i += RS_BLOCK) kys[i] = p.k_y[(long long)oy0 * p.ksize_y + i];

    const long long src_bytes = (long long)(p.N - 1) * p.src_frame_stride + 3LL * p.Hin * p.Win;
    const long long seg_at = (long long)f * p.src_frame_stride + 3LL * seg_lo;      // + row * 3 Win: a row segment's first byte
    const int seg_bytes = 3 * (seg_hi - seg_lo);
    const int row_bytes = 3 * p.Win;
    const uint32_t* src_dw = reinterpret_cast<const uint32_t*>(p.src);
    const int pieces = (g.seg_dw_cap + 63) >> 6;              // wave-wide pieces of a row segment

    for (int r0 = y0; r0 < y1; r0 += g.raw_rows) {
        const int rows = min(g.raw_rows, y1 - r0);
        __syncthreads();                                      // the tables (first round); the previous chunk's raw rows are read
        // stage-in: unit u = (row, piece); a wave takes four units at a time and has their loads in flight together
        const int units = rows * pieces;
        for (int u = wave; u < units; u += RS_WAVES * RS_STAGE) {
            uint32_t v[RS_STAGE];
            int at[RS_STAGE];
#pragma unroll
            for (int j = 0; j < RS_STAGE; ++j) {
                const int uu = u + j * RS_WAVES;
                at[j] = -1;
                if (uu < units) {
                    const int rl = uu / pieces, d = (uu - rl * pieces) * 64 + lane;
                    const long long begin = seg_at + (long long)(r0 + rl) * row_bytes;
                    const long long d0 = begin >> 2, d1 = (begin + seg_bytes + 3) >> 2;
                    if (d0 + d < d1) {
                        const long long b = (d0 + d) * 4;
                        at[j] = rl * g.seg_dw_cap + d;
                        if (b + 4 <= src_bytes) {
                            v[j] = src_dw[d0 + d];
                        } else {                              // the array's last dword where its size is no multiple of 4
                            uint32_t w = 0;
                            for (int e = 0; e < 4; ++e)
                                if (b + e < src_bytes) w |= (uint32_t)p.src[b + e] << (8 * e);
                            v[j] = w;
                        }
                    }
                }
            }
#pragma unroll
            for (int j = 0; j < RS_STAGE; ++j)
                if (at[j] >= 0) raw[at[j]] = v[j];
        }
        __syncthreads();
        // horizontal pass: (row of the chunk, tile column) -> three bytes of the intermediate tile
        for (int i = tid; i < rows * tw; i += RS_BLOCK) {
            const int rl = tw == RS_TX ? i / RS_TX : i / tw, t = i - rl * tw;
            const int off = (int)((seg_at + (long long)(r0 + rl) * row_bytes) & 3);
            const uint8_t* rp = reinterpret_cast<const uint8_t*>(raw + rl * g.seg_dw_cap) + off + 3 * sxs[t];
            int c0, c1, c2;
            if (hcopy) {
                c0 = rp[0], c1 = rp[1], c2 = rp[2];
            } else {
                const int n = cxs[t];
                const int* k = kxs + t * p.ksize_x;
                int a0 = 1 << (RS_PRECISION - 1), a1 = a0, a2 = a0;
                for (int x = 0; x < n; ++x) {
                    const int kk = k[x];
                    a0 += rp[3 * x] * kk, a1 += rp[3 * x + 1] * kk, a2 += rp[3 * x + 2] * kk;
                }
                c0 = rs_clip8(a0), c1 = rs_clip8(a1), c2 = rs_clip8(a2);   // rounded to bytes here, as Pillow's intermediate image is
            }
            uint8_t* m = mid + (r0 - y0 + rl) * RS_MID_ROW + 3 * t;
            m[0] = (uint8_t)c0, m[1] = (uint8_t)c1, m[2] = (uint8_t)c2;
        }
    }
    __syncthreads();
    // vertical pass: (tile row, dword of its output row segment) -> up to four bytes of dst
    uint8_t* dst = p.dst + (long long)f * p.dst_frame_stride;
    for (int i = tid; i < th * RS_OUT_DW; i += RS_BLOCK) {
        const int ol = i / RS_OUT_DW, dl = i - ol * RS_OUT_DW;
        const int B = ((oy0 + ol) * p.W + ox0) * 3, E = B + 3 * tw;        // (3 H W < 2^31)
        const int at = ((B >> 2) + dl) * 4;
        if (at >= E) continue;
        const uint8_t* mp = mid + sys[ol] * RS_MID_ROW;
        const int n = cys[ol];
        const int* k = kys + ol * p.ksize_y;
        int j[4], out[4];
        bool in[4];
#pragma unroll
        for (int b = 0; b < 4; ++b) {
            j[b] = at + b - B;
            in[b] = j[b] >= 0 && j[b] < 3 * tw;
            j[b] = rs_clamp(j[b], 0, 3 * tw - 1);
        }
        if (vcopy) {
#pragma unroll
            for (int b = 0; b < 4; ++b) out[b] = mp[j[b]];
        } else {
            int a[4];
#pragma unroll
            for (int b = 0; b < 4; ++b) a[b] = 1 << (RS_PRECISION - 1);
            for (int y = 0; y < n; ++y) {
                const int kk = k[y];
#pragma unroll
                for (int b = 0; b < 4; ++b) a[b] += mp[y * RS_MID_ROW + j[b]] * kk;
            }
#pragma unroll
            for (int b = 0; b < 4; ++b) out[b] = rs_clip8(a[b]);
        }
        if (in[0] && in[3]) {
            *reinterpret_cast<uint32_t*>(dst + at) = (uint32_t)out[0] | ((uint32_t)out[1] << 8) | ((uint32_t)out[2] << 16) | ((uint32_t)out[3] << 24);
        } else {
#pragma unroll
            for (int b = 0; b < 4; ++b)
                if (in[b]) dst[at + b] = (uint8_t)out[b];
        }
    }
}

// Input pixels the taps of T consecutive output pixels can span: start > center - support - 0.5 at the first, start + count <= center + support
// + 0.5 at the last, (T - 1) * scale between the two centres; two more for the roundings of this very expression.
static int span_cap(int T, int in, int out) {
    if (in == out) return T;
    const double scale = (double)in / out, fs = scale < 1.0 ? 1.0 : scale;
    const long long c = (long long)((T - 1) * scale + 2.0 * fs + 1.0) + 2;
    return (int)(c < in ? c : in);
}

static double tri(double a) {
    if (a < 0.0) a = -a;
    return a < 1.0 ? 1.0 - a : 0.0;
}

}  // namespace ucnerf

using namespace ucnerf;

extern "C" {

int ucnerf_resize_bilinear_ksize(int in, int out) {
    UCNERF_REQUIRE(in >= 1 && out >= 1 && in <= (1 << 24) && out <= (1 << 24), "resize_bilinear_ksize: in = %d, out = %d outside 1 .. 2^24", in, out);
    const double scale = (double)in / out, fs = scale < 1.0 ? 1.0 : scale;
    const double support = 1.0 * fs;
    return (int)ceil(support) * 2 + 1;
}

int ucnerf_resize_bilinear_coeffs(int in, int out, int32_t* start, int32_t* count, int32_t* k) {
    const int ksize = ucnerf_resize_bilinear_ksize(in, out);
    if (ksize < 0) return ksize;
    UCNERF_REQUIRE(start && count && k, "resize_bilinear_coeffs: null start, count or k");
    const double scale = (double)in / out, fs = scale < 1.0 ? 1.0 : scale;
    const double support = 1.0 * fs, ss = 1.0 / fs;
    for (int xx = 0; xx < out; ++xx) {
        const double center = (xx + 0.5) * scale;
        int xmin = (int)(center - support + 0.5);
        if (xmin < 0) xmin = 0;
        int xmax = (int)(center + support + 0.5);
        if (xmax > in) xmax = in;
        const int n = xmax - xmin;
        // (no scratch array: the weights are formed twice, the same expression giving the same double both times)
        double ww = 0.0;
        for (int x = 0; x < n; ++x) ww += tri((x + xmin - center + 0.5) * ss);
        int32_t* kk = k + (long long)xx * ksize;
        for (int x = 0; x < n; ++x) {
            double w = tri((x + xmin - center + 0.5) * ss);
            if (ww != 0.0) w /= ww;
            kk[x] = w < 0.0 ? (int)(-0.5 + w * (double)(1 << RS_PRECISION)) : (int)(0.5 + w * (double)(1 << RS_PRECISION));
        }
        for (int x = n; x < ksize; ++x) kk[x] = 0;
        start[xx] = xmin;
        count[xx] = n;
    }
    return ksize;
}

int ucnerf_resize_bilinear_u8(const ucnerf_resize_params* p, void* stream) {
    UCNERF_REQUIRE(p, "resize_bilinear_u8: null params");
    UCNERF_REQUIRE(p->N >= 0, "resize_bilinear_u8: N = %d (negative)", p->N);
    if (p->N == 0) return UCNERF_OK;                          // an empty batch: nothing launched, no pointer looked at
    UCNERF_REQUIRE(p->Hin >= 1 && p->Win >= 1 && p->H >= 1 && p->W >= 1, "resize_bilinear_u8: %d x %d -> %d x %d (a size below 1)", p->Hin, p->Win, p->H, p->W);
    UCNERF_REQUIRE(p->Hin <= RS_MAX_SIZE && p->Win <= RS_MAX_SIZE && p->H <= RS_MAX_SIZE && p->W <= RS_MAX_SIZE && 3LL * p->Hin * p->Win < (1LL << 31) &&
                   3LL * p->H * p->W < (1LL << 31), "resize_bilinear_u8: %d x %d -> %d x %d (a size above %d, or a frame of 2^31 bytes)", p->Hin, p->Win, p->H,
                   p->W, RS_MAX_SIZE);
    UCNERF_REQUIRE(p->N <= 65535, "resize_bilinear_u8: N = %d frames above 65535", p->N);
    UCNERF_REQUIRE(p->src && p->dst && p->start_x && p->count_x && p->k_x && p->start_y && p->count_y && p->k_y,
                   "resize_bilinear_u8: null src, dst or coefficient table (start_x, count_x, k_x, start_y, count_y, k_y)");
    UCNERF_REQUIRE(p->src_frame_stride >= 3LL * p->Hin * p->Win, "resize_bilinear_u8: src_frame_stride = %lld below 3 Hin Win = %lld", (long long)p->src_frame_stride,
                   3LL * p->Hin * p->Win);
    UCNERF_REQUIRE((p->dst_frame_stride & 3) == 0 && p->dst_frame_stride >= 3LL * p->H * p->W,
                   "resize_bilinear_u8: dst_frame_stride = %lld must be a multiple of 4 and at least 3 H W = %lld", (long long)p->dst_frame_stride, 3LL * p->H * p->W);
    UCNERF_REQUIRE((((uintptr_t)p->src | (uintptr_t)p->dst) & 3) == 0, "resize_bilinear_u8: src and dst must be 4-byte aligned (their bytes move as dwords)");
    UCNERF_REQUIRE(p->ksize_x == ucnerf_resize_bilinear_ksize(p->Win, p->W) && p->ksize_y == ucnerf_resize_bilinear_ksize(p->Hin, p->H),
                   "resize_bilinear_u8: ksize_x = %d, ksize_y = %d are not the ksize of %d -> %d (%d) and %d -> %d (%d)", p->ksize_x, p->ksize_y, p->Win, p->W,
                   ucnerf_resize_bilinear_ksize(p->Win, p->W), p->Hin, p->H, ucnerf_resize_bilinear_ksize(p->Hin, p->H));
    UCNERF_REQUIRE((long long)p->Win <= (long long)UCNERF_RESIZE_MAX_RATIO * p->W && (long long)p->Hin <= (long long)UCNERF_RESIZE_MAX_RATIO * p->H,
                   "resize_bilinear_u8: %d x %d -> %d x %d shrinks an axis by more than the ratio %d (a workgroup's tile would not fit in LDS)", p->Hin, p->Win,
                   p->H, p->W, UCNERF_RESIZE_MAX_RATIO);
    ResizeGeom g;
    g.seg_cols_cap = span_cap(RS_TX, p->Win, p->W);
    g.seg_dw_cap = (3 * g.seg_cols_cap + 3 + 3) / 4;          // a segment may start at byte 3 of its first dword
    g.mid_rows_cap = span_cap(RS_TY, p->Hin, p->H);
    const long long fixed = 4LL * (RS_TX * p->ksize_x + RS_TY * p->ksize_y + 2 * RS_TX + 2 * RS_TY) + (long long)g.mid_rows_cap * RS_MID_ROW;
    long long rows = (RS_LDS_TARGET - fixed) / (4LL * g.seg_dw_cap);
    g.raw_rows = (int)(rows < 1 ? 1 : (rows > g.mid_rows_cap ? g.mid_rows_cap : rows));
    const long long lds = fixed + 4LL * g.raw_rows * g.seg_dw_cap;
    UCNERF_REQUIRE(lds <= RS_LDS_MAX, "resize_bilinear_u8: %d x %d -> %d x %d needs %lld bytes of LDS per workgroup (at most %d)", p->Hin, p->Win, p->H, p->W,
                   lds, RS_LDS_MAX);

    hipLaunchKernelGGL(resize_bilinear_u8_kernel, dim3(cdiv(p->W, RS_TX), cdiv(p->H, RS_TY), p->N), dim3(RS_BLOCK), (size_t)lds, (hipStream_t)stream, *p, g);
    return check_launch("resize_bilinear_u8");
}

}  // extern "C"
