// slide.hip -- sliding-window dense inference (dinov2_hip_predict_dense_slide, include/dinov2_hip.h) for gfx950 (MI355X).
//
// No reference counterpart: mmsegmentation's slide_inference (test_cfg mode='slide') around a linear head on frozen features.  Two kernels around
// the ordinary forward and head (csrc/dense.hip):
//   slide_gather_kernel  copies every window out of the resident images into one contiguous window batch of the same layout, four bytes at a
//                        time: window starts are arbitrary, so neither side of the copy has more than the alignment of a float.
//   slide_reduce_kernel  a workgroup owns a tile of output pixels in IMAGE coordinates, stages the low-resolution logit rows that the tile needs
//                        of every window touching it into LDS, and every thread walks the classes of its pixel: per class the bilinear
//                        interpolation inside each covering window (ascending window index), their f32 sum, the division by their number;
//                        then the running argmax (ARGMAX) or the two running sums of the bins (BINS).  Neither the full-resolution logit
//                        planes nor their per-window resamplings ever exist.
// Everything the contract fixes bit for bit is written as separate f32 operations under `fp contract(off)`.
#include "device_types.h"
#include "kernels.h"

namespace dinov2 {

// Workgroup (x, y): elements [256 x, +256) of window y of the batch.  An element is one float of the window in its own layout.
__global__ __launch_bounds__(256) void slide_gather_kernel(const float* __restrict__ img, float* __restrict__ win, const int* __restrict__ tab, int h,
                                                           int w, int ny, int nx, int ch, int cw, int chw) {
    const int nwin = ny * nx;
    const int b = blockIdx.y / nwin, k = blockIdx.y - b * nwin;
    const int iy = k / nx, ix = k - iy * nx;
    const int y1 = tab[iy], x1 = tab[ny + ix];
    if (y1 < 0 || x1 < 0 || y1 + ch > h || x1 + cw > w) return;  // (uniform; a table that is not this image's copies nothing)
    const size_t per = (size_t)3 * ch * cw, e = (size_t)blockIdx.x * 256 + threadIdx.x;
    if (e >= per) return;
    const float* const src = img + (size_t)b * 3 * h * w;
    size_t s;
    if (chw) {
        const size_t plane = (size_t)ch * cw, c = e / plane, r = e - c * plane;
        const size_t y = r / cw, x = r - y * cw;
        s = (c * h + y1 + y) * w + x1 + x;
    } else {
        const size_t line = (size_t)cw * 3, y = e / line, r = e - y * line;
        s = ((size_t)(y1 + y) * w + x1) * 3 + r;
    }
    win[(size_t)blockIdx.y * per + e] = src[s];
}

hipError_t launch_slide_gather(const float* img, float* win, const int* tab, int B, int h, int w, int ny, int nx, int crop_h, int crop_w, int layout,
                               hipStream_t st) {
    if (!img || !win || !tab || B < 1 || ny < 1 || nx < 1 || crop_h < 1 || crop_w < 1 || crop_h > h || crop_w > w) return hipErrorInvalidValue;
    if (layout != 0 && layout != 1) return hipErrorInvalidValue;
    const long long windows = (long long)B * ny * nx, blocks = ((long long)3 * crop_h * crop_w + 255) / 256;
    if (windows > SLIDE_WINDOWS_MAX || blocks > 0x7fffffffLL) return hipErrorInvalidValue;
    hipLaunchKernelGGL(slide_gather_kernel, dim3((unsigned)blocks, (unsigned)windows), dim3(256), 0, st, img, win, tab, h, w, ny, nx, crop_h, crop_w,
                       layout);
    return hipGetLastError();
}

// what slide_reduce_kernel takes of a SlideReducePlan
struct SlideGeom {
    int ty, tx, sy, sx, ry, rx, chunk, pitch;
    float scale_y, scale_x;
};

namespace {

// One axis of a tile, by the first threads of the workgroup: meta[s] = (start of the tile's window s, first staged row, staged rows, -) and
// entry[l * slots + s] = (i0, i1 relative to that first row, lambda's bits, 1) where window s covers coordinate p0 + l, (0, 0, 0, 0) elsewhere.
__device__ __forceinline__ void slide_axis_tables(int tid, const int* __restrict__ starts, int lo, int n, int slots, int p0, int npx, int tile, int crop,
                                                  int n_in, int span, float scale, int4* __restrict__ meta, int4* __restrict__ entry) {
    for (int i = tid; i < tile * slots; i += 256) {
        const int l = i / slots, s = i - l * slots;
        int4 e = {0, 0, 0, 0};
        if (l < npx && s < n) {
            const int ws = starts[lo + s], d = p0 + l - ws;
            if (d >= 0 && d < crop) {
                const int d0 = p0 > ws ? p0 - ws : 0;
                int first, i0, i1, unused;
                float lam;
                dense_axis(scale, d0, n_in, first, unused, lam);
                dense_axis(scale, d, n_in, i0, i1, lam);
                e = int4{i0 - first, i1 - first, __float_as_int(lam), 1};
            }
        }
        entry[i] = e;
    }
    for (int s = tid; s < slots; s += 256) {
        int4 m = {0, 0, 0, 0};
        if (s < n) {
            const int ws = starts[lo + s];
            const int d0 = p0 > ws ? p0 - ws : 0, d1 = p0 + npx - 1 - ws < crop - 1 ? p0 + npx - 1 - ws : crop - 1;
            int first, last, unused;
            float lam;
            dense_axis(scale, d0, n_in, first, unused, lam);
            dense_axis(scale, d1, n_in, unused, last, lam);
            const int rows = last - first + 1;
            m = int4{ws, first, rows < span ? rows : span, 0};
        }
        meta[s] = m;
    }
}

}  // namespace

// Workgroup (x, y, z): output pixels [y ty, +ty) x [x tx, +tx) of image z, pixel to thread row-major (a wave's lanes are neighbours in x, as in
// dense_reduce_kernel).  Dynamic LDS: the staged rows [sy][sx][ry][rx][pitch] f32 of one class chunk, the centres [C to a multiple of 4], the
// two axis tables, the tile's labels.  tab: y1 | x1 | tile rows' window ranges | tile columns' (kernels.h slide_table_fill).
// Orders (contract 3 and 4): per class the covering windows ascend (window rows outside, columns inside: k = iy nx + ix), the classes ascend
// within a chunk and the chunks ascend, the pixel's running state living in registers from chunk to chunk.
template <int REDUCE>
__global__ __launch_bounds__(256) void slide_reduce_kernel(const float* __restrict__ L, int ldl, int h0, int w0, int C, int ch, int cw, int h, int w,
                                                           int ny, int nx, const int* __restrict__ tab, SlideGeom g,
                                                           const float* __restrict__ centers, float eps, uint8_t* __restrict__ labels,
                                                           float* __restrict__ value) {
#pragma clang fp contract(off)  // contract 3 and 4: every multiplication, addition and division rounds on its own
    extern __shared__ __attribute__((aligned(16))) float slide_lds[];
    const int tid = threadIdx.x;
    const int C4 = (C + 3) >> 2, pitch4 = g.pitch >> 2;
    const int slot_rows = g.ry * g.rx;
    float4* const rows4 = (float4*)slide_lds;
    float* const cen = slide_lds + (size_t)g.sy * g.sx * slot_rows * g.pitch;
    int4* const ytab = (int4*)(cen + 4 * C4);
    int4* const xtab = ytab + g.ty * g.sy;
    int4* const ymeta = xtab + g.tx * g.sx;
    int4* const xmeta = ymeta + g.sy;
    uint8_t* const lab = (uint8_t*)(xmeta + g.sx);
    const int y_first = blockIdx.y * g.ty, x_first = blockIdx.x * g.tx;
    const int ny_px = h - y_first < g.ty ? h - y_first : g.ty, nx_px = w - x_first < g.tx ? w - x_first : g.tx;
    const int* const yr = tab + ny + nx + 2 * blockIdx.y;
    const int* const xr = tab + ny + nx + 2 * gridDim.y + 2 * blockIdx.x;
    const int wy_lo = yr[0], nsy = yr[1], wx_lo = xr[0], nsx = xr[1];
    // (uniform; the planner's slots cover every tile, and a table that is not this launch's reads no window that does not exist)
    if (nsy < 1 || nsx < 1 || nsy > g.sy || nsx > g.sx || wy_lo < 0 || wx_lo < 0 || wy_lo + nsy > ny || wx_lo + nsx > nx) return;
    slide_axis_tables(tid, tab, wy_lo, nsy, g.sy, y_first, ny_px, g.ty, ch, h0, g.ry, g.scale_y, ymeta, ytab);
    slide_axis_tables(tid, tab + ny, wx_lo, nsx, g.sx, x_first, nx_px, g.tx, cw, w0, g.rx, g.scale_x, xmeta, xtab);
    if (REDUCE == DENSE_BINS)
        for (int i = tid; i < C; i += 256) cen[i] = centers[i];
    __syncthreads();

    const int ly = tid / g.tx, lx = tid - ly * g.tx;
    const bool active = ly < ny_px && lx < nx_px;  // (ly < ty follows: ny_px <= ty)
    const int4* const yrow = ytab + (active ? ly : 0) * g.sy;
    const int4* const xrow = xtab + (active ? lx : 0) * g.sx;
    float nf = 1.0f;
    if (active) {
        int cy = 0, cx = 0;
        for (int s = 0; s < nsy; ++s) cy += yrow[s].w;
        for (int s = 0; s < nsx; ++s) cx += xrow[s].w;
        nf = (float)(cy * cx);
    }
    const size_t P = (size_t)h0 * w0;
    const float* const Lb = L + (size_t)blockIdx.z * ny * nx * P * ldl;
    const int wave = tid >> 6, lane = tid & 63;
    float best = 0.0f, S = 0.0f, D = 0.0f;
    int bi = 0;
    for (int c0 = 0; c0 < C; c0 += g.chunk) {
        const int ncls = C - c0 < g.chunk ? C - c0 : g.chunk;
        if (c0) __syncthreads();  // (everyone has left the previous chunk's rows)
        // stage: a wave per row (its place is wave-uniform arithmetic), the lanes along the classes
        for (int r = wave; r < nsy * nsx * slot_rows; r += 4) {
            const int slot = r / slot_rows, rr = r - slot * slot_rows;
            const int s_y = slot / nsx, s_x = slot - s_y * nsx;
            const int ry = rr / g.rx, rx = rr - ry * g.rx;
            const int4 my = ymeta[s_y], mx = xmeta[s_x];
            if (ry >= my.z || rx >= mx.z) continue;  // (uniform: this window needs fewer rows than the widest)
            const size_t win = (size_t)(wy_lo + s_y) * nx + wx_lo + s_x;
            const float* const src = Lb + (win * P + (size_t)(my.y + ry) * w0 + mx.y + rx) * ldl + c0;
            float* const dst = slide_lds + (size_t)((s_y * g.sx + s_x) * slot_rows + rr) * g.pitch;
            for (int c = lane; c < ncls; c += 64) dst[c] = src[c];
        }
        __syncthreads();
        if (!active) continue;
        auto reduce_one = [&](int cls, float acc) {
            const float mean = acc / nf;
            if (REDUCE == DENSE_ARGMAX) {
                if (cls == 0 || mean > best) {  // strictly greater: equal values (-0 and +0 among them) stay with the lowest class
                    best = mean;
                    bi = cls;
                }
            } else {
                const float r = (mean > 0.0f ? mean : 0.0f) + eps;
                S = S + r;
                D = D + r * cen[cls];
            }
        };
        const int nq = (ncls + 3) >> 2;
        for (int q = 0; q < nq; ++q) {  // four classes per 16-byte read of each neighbour row
            float a0 = -0.0f, a1 = -0.0f, a2 = -0.0f, a3 = -0.0f;  // (-0 + v has the bits of v, the sign of a zero included: "starts as the first")
            for (int s_y = 0; s_y < nsy; ++s_y) {
                const int4 ye = yrow[s_y];
                if (!ye.w) continue;
                const float ay = __int_as_float(ye.z), by = 1.0f - ay;
                for (int s_x = 0; s_x < nsx; ++s_x) {
                    const int4 xe = xrow[s_x];
                    if (!xe.w) continue;
                    const float ax = __int_as_float(xe.z), bx = 1.0f - ax;
                    const float4* const base = rows4 + (size_t)(s_y * g.sx + s_x) * slot_rows * pitch4 + q;
                    const float4 v00 = base[(ye.x * g.rx + xe.x) * pitch4], v01 = base[(ye.x * g.rx + xe.y) * pitch4];
                    const float4 v10 = base[(ye.y * g.rx + xe.x) * pitch4], v11 = base[(ye.y * g.rx + xe.y) * pitch4];
                    auto val = [&](float p00, float p01, float p10, float p11) {
                        const float t = bx * p00 + ax * p01;
                        const float u = bx * p10 + ax * p11;
                        return by * t + ay * u;
                    };
                    a0 = a0 + val(v00.x, v01.x, v10.x, v11.x);
                    a1 = a1 + val(v00.y, v01.y, v10.y, v11.y);
                    a2 = a2 + val(v00.z, v01.z, v10.z, v11.z);
                    a3 = a3 + val(v00.w, v01.w, v10.w, v11.w);
                }
            }
            const int cls = c0 + 4 * q, left = C - cls;  // (uniform) what lies behind the last class in a row is never reduced
            reduce_one(cls, a0);
            if (left > 1) reduce_one(cls + 1, a1);
            if (left > 2) reduce_one(cls + 2, a2);
            if (left > 3) reduce_one(cls + 3, a3);
        }
    }
    const size_t img = (size_t)blockIdx.z * h;
    if (active) {
        const size_t o = (img + y_first + ly) * w + x_first + lx;
        if (REDUCE == DENSE_ARGMAX) {
            lab[ly * g.tx + lx] = (uint8_t)bi;
            if (value) value[o] = best;
        } else {
            value[o] = D / S;
        }
    }
    if (REDUCE != DENSE_ARGMAX || !labels) return;  // (uniform)
    __syncthreads();
    // the tile's labels as in dense_reduce_kernel: every row's run of nx_px bytes leaves as aligned 32-bit words, the ends as single bytes
    const int words = (g.tx + 3) / 4 + 1;
    for (int i = tid; i < ny_px * words; i += 256) {
        const int row = i / words, wi = i - row * words;
        uint8_t* const gp = labels + (img + y_first + row) * w + x_first;
        const int off = 4 * wi - (int)((uintptr_t)gp & 3);  // of the word's first byte within the run: -3 .. nx_px + 3
        uint8_t* const wa = gp + off;
        if (off >= 0 && off + 3 < nx_px) {
            const uint8_t* const s = lab + row * g.tx + off;
            *(unsigned*)wa = (unsigned)s[0] | ((unsigned)s[1] << 8) | ((unsigned)s[2] << 16) | ((unsigned)s[3] << 24);
        } else {
            for (int k = 0; k < 4; ++k)
                if (off + k >= 0 && off + k < nx_px) wa[k] = lab[row * g.tx + off + k];
        }
    }
}

hipError_t launch_slide_reduce(const float* logits, int ldl, int B, int h0, int w0, int C, int crop_h, int crop_w, int h, int w, int ny, int nx,
                               const int* tab, int reduce, const float* centers, float eps, uint8_t* labels, float* value, const SlideReducePlan& p,
                               hipStream_t st) {
    if (!logits || !tab || B < 1 || ny < 1 || nx < 1 || (long long)B * ny * nx > SLIDE_WINDOWS_MAX || ldl < C || ((size_t)logits & 3) != 0)
        return hipErrorInvalidValue;
    if (h0 < 1 || w0 < 1 || C < 1 || C > DENSE_C_MAX || crop_h < 1 || crop_w < 1 || crop_h > h || crop_w > w || h > DENSE_OUT_MAX || w > DENSE_OUT_MAX)
        return hipErrorInvalidValue;
    if (reduce != DENSE_ARGMAX && reduce != DENSE_BINS) return hipErrorInvalidValue;
    if (reduce == DENSE_BINS && (!centers || !value || labels || !(eps > 0.0f))) return hipErrorInvalidValue;
    if (reduce == DENSE_ARGMAX && !labels && !value) return hipErrorInvalidValue;
    // the plan must be one slide_reduce_plan gives (the starts are the caller's: the kernel checks what it reads of the table against the slots)
    if (p.tile_y < 1 || p.tile_x < 1 || p.tile_y * p.tile_x > 256 || p.slots_y < 1 || p.slots_x < 1 || p.span_y < 1 || p.span_x < 1 ||
        p.chunk < 4 || p.chunk % 4 != 0 || p.pitch != dense_pitch(p.chunk) || p.grid_y != (h + p.tile_y - 1) / p.tile_y ||
        p.grid_x != (w + p.tile_x - 1) / p.tile_x || p.scale_y != (float)h0 / (float)crop_h || p.scale_x != (float)w0 / (float)crop_w ||
        p.lds_bytes != slide_lds_bytes(p.tile_y, p.tile_x, p.slots_y, p.slots_x, p.span_y, p.span_x, p.pitch, C) || p.lds_bytes > DENSE_LDS_BUDGET)
        return hipErrorInvalidValue;
    const dim3 grid((unsigned)p.grid_x, (unsigned)p.grid_y, (unsigned)B), block(256);
    const SlideGeom g{p.tile_y, p.tile_x, p.slots_y, p.slots_x, p.span_y, p.span_x, p.chunk, p.pitch, p.scale_y, p.scale_x};
    if (reduce == DENSE_ARGMAX)
        hipLaunchKernelGGL(slide_reduce_kernel<DENSE_ARGMAX>, grid, block, p.lds_bytes, st, logits, ldl, h0, w0, C, crop_h, crop_w, h, w, ny, nx, tab,
                           g, centers, eps, labels, value);
    else
        hipLaunchKernelGGL(slide_reduce_kernel<DENSE_BINS>, grid, block, p.lds_bytes, st, logits, ldl, h0, w0, C, crop_h, crop_w, h, w, ny, nx, tab, g,
                           centers, eps, labels, value);
    return hipGetLastError();
}

}  // namespace dinov2
