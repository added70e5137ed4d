// ss_redact.hip — redaction of regions of resident BGR u8 frames, in place: box blur, pixelation or a colour fill over rectangles,
// ellipses and polygons (docs/REDACT.md; the bytes are those of tests/redact_ref.py).  The frames every `--save` run writes show the
// people it tracks; this is the pixel work that hides them before the overlay draws on top.
//
// Every output pixel is a function of the UNTOUCHED frame, so overlapping regions, their order and a region cut in two give the
// same bytes.  A blur reads a neighbourhood, so a tile may not be written while a neighbour still reads it: three launches in
// stream order, with no copy of the frame —
//   k_redact_tiles    one thread per (frame, 64 x 32 tile): does a region's clipped bounding box meet it?  The hits go to a work list
//                     (vector atomicAdd on its length; the list's order decides no byte).
//   k_redact_compute  a fixed grid strides over the list, one 256-thread workgroup per tile: the tile and its halo of r pixels go to
//                     LDS (reflect-101 resolved while loading, aligned 4-byte loads inside the row), column sums run down the rows
//                     into u16, four columns a thread (63 * 255 fits), row sums over them in registers, one multiply-shift per byte (ss_redact_div.h);
//                     coverage once per pixel over the tile's own region sublist; the bytes and one coverage bit per pixel go to the
//                     tile's slot in the scratch.  Pixelation: the same body with cell sums (cells never cross a tile: their size
//                     divides 64 and 32 and they start at the frame's origin).  Fill loads nothing.
//   k_redact_store    the covered pixels of every listed tile, from its slot to the frame.  Every read of the frame is in the
//                     launch before.
// Traffic: the touched tiles and their halos, once in and the covered pixels once out.  The scratch is sized for every tile of
// every frame (ss_redact_scratch_bytes) but only the listed tiles' slots are touched.
#include "ss_common.h"
#include "ss_cover.h"
#include "ss_launch.h"
#include "ss_redact_div.h"

#define RD_RECT 0              // inclusive corners (x0,y0)-(x1,y1) in any order, clipped to the frame
#define RD_ELLIPSE 1           // inscribed in that clipped rectangle
#define RD_POLY 2              // even-odd interior (OV_POLY) united with the thickness-2 OV_LINE coverage of every edge; (x0,y0)-(x1,y1): the
                               // vertices' bounding box, voff: first vertex (x, y pairs) in the vertex array, nv vertices; nv < 3 covers nothing
#define RD_BLUR 0
#define RD_PIXELATE 1
#define RD_FILL 2
#define RD_TW 64
#define RD_TH 32
#define RD_MAXREG 1024         // regions a frame
#define RD_MAXV 4096           // vertices a polygon (yolo.py traces outlines of up to 2048 points on the device, longer ones on the host)
#define RD_MAXSIDE 8192
#define RD_PIX (RD_TW * RD_TH * 3)
#define RD_SLOT (RD_PIX + RD_TH * 8)        // a tile's result bytes, then one coverage byte per 8 pixels
#define RD_HEAD 2064           // LDS: u16 hits[1024], the hit count
#define RD_LIST_AT 256         // scratch: the list's length, then the list, then the slots

struct RdRegion { int type, x0, y0, x1, y1, voff, nv, pad; };

// the region's bounding box clipped to the frame; false: it covers nothing
__device__ __forceinline__ bool rd_bbox(const RdRegion& g, int H, int W, int& bx0, int& by0, int& bx1, int& by1)
{
    if (g.type < RD_RECT || g.type > RD_POLY) return false;
    const int e = g.type == RD_POLY ? 1 : 0;                        // a polygon's edges are 2 thick: one pixel beyond the vertices
    if (e && g.nv < 3) return false;
    bx0 = max(min(g.x0, g.x1), e) - e; by0 = max(min(g.y0, g.y1), e) - e;
    bx1 = min(max(g.x0, g.x1), W - 1 - e) + e; by1 = min(max(g.y0, g.y1), H - 1 - e) + e;
    return bx0 <= bx1 && by0 <= by1;
}

// (x, y) is a pixel of the frame
__device__ __forceinline__ bool rd_covers(const RdRegion& g, int x, int y, int H, int W, const int* __restrict__ verts)
{
    int X0, Y0, X1, Y1;
    if (!rd_bbox(g, H, W, X0, Y0, X1, Y1)) return false;
    if (x < X0 || x > X1 || y < Y0 || y > Y1) return false;
    if (g.type == RD_RECT) return true;
    if (g.type == RD_ELLIPSE) {
        const long long a = X1 - X0 + 1, b = Y1 - Y0 + 1, u = 2 * x - X0 - X1, v = 2 * y - Y0 - Y1;
        return u * u * b * b + v * v * a * a <= a * a * b * b;       // sides <= 8192: below 2^54
    }
    const int n = min(g.nv, RD_MAXV);
    const uint8_t* pts = reinterpret_cast<const uint8_t*>(verts + 2 * (size_t)g.voff);
    OvPrim q = {OV_POLY, x, y, x, y, 0, 0, n << 1};                  // (its own bounding-box test passes: the one above has been made)
    if (ov_covers(q, x, y, pts, nullptr)) return true;
    const int* pv = reinterpret_cast<const int*>(pts);
    int ax = pv[2 * (n - 1)], ay = pv[2 * (n - 1) + 1];
    for (int i = 0; i < n; ++i) {
        const int bx = pv[2 * i], by = pv[2 * i + 1];
        OvPrim l = {OV_LINE, ax, ay, bx, by, 0, 2, 0};
        if (ov_covers(l, x, y, nullptr, nullptr)) return true;
        ax = bx; ay = by;
    }
    return false;
}

__device__ __forceinline__ bool rd_meets(const RdRegion& g, int H, int W, int X, int Y)
{
    int bx0, by0, bx1, by1;
    return rd_bbox(g, H, W, bx0, by0, bx1, by1) && bx1 >= X && bx0 < X + RD_TW && by1 >= Y && by0 < Y + RD_TH;
}

__global__ __launch_bounds__(256) void k_redact_tiles(const RdRegion* __restrict__ regs, const int* __restrict__ reg_off, int total, int H, int W, int tx,
                                                      int tiles, int* __restrict__ count, unsigned* __restrict__ list)
{
    const long long id = (long long)blockIdx.x * 256 + threadIdx.x;
    if (id >= total) return;
    const int b = (int)(id / tiles), t = (int)(id % tiles), X = (t % tx) * RD_TW, Y = (t / tx) * RD_TH;
    const int r0 = reg_off[b], r1 = min(reg_off[b + 1], r0 + RD_MAXREG);
    bool hit = false;
    for (int i = r0; i < r1 && !hit; ++i) hit = rd_meets(regs[i], H, W, X, Y);
    if (hit) list[atomicAdd(count, 1)] = (unsigned)id;
}

// hh rows of hw pixels from (X0, Y0) of the frame into LDS, halo byte h of row j at raw[j * pitch + h] (pitch: 3 hw rounded up to 4).
// Inside the row a 4-byte word of LDS comes from one aligned 4-byte load, or from two shifted together where the row starts at
// another alignment; outside the frame: reflect-101 (reflect) or zeros, byte by byte.
__device__ __forceinline__ void rd_load(uint8_t* raw, int pitch, const uint8_t* __restrict__ frame, int H, int W, int rs, int X0, int Y0, int hw, int hh,
                                        bool reflect, int tid)
{
    const int upr = pitch >> 2;
    const long long gb0 = (long long)X0 * 3;
    for (int u = tid; u < hh * upr; u += 256) {
        const int j = u / upr, q = u - j * upr, h0 = 4 * q;
        int sy = Y0 + j;
        const bool row_in = sy >= 0 && sy < H;
        if (!row_in) sy = reflect ? ss_redact_reflect(sy, H) : 0;
        const uint8_t* rowp = frame + (size_t)sy * rs;
        const long long g0 = gb0 + h0;                               // the word's first byte in the row
        uint32_t word = 0;
        if (row_in || reflect) {
            if (h0 + 3 < 3 * hw && g0 >= 0 && g0 + 3 < 3LL * W) {    // four bytes of the row as they lie
                const uint8_t* g = rowp + g0;
                const int sh = (int)((uintptr_t)g & 3);
                if (sh == 0) word = *reinterpret_cast<const uint32_t*>(g);
                else if (g0 - sh >= 0 && g0 - sh + 7 < 3LL * W) {
                    const uint32_t lo = *reinterpret_cast<const uint32_t*>(g - sh), hi = *reinterpret_cast<const uint32_t*>(g - sh + 4);
                    word = (lo >> (8 * sh)) | (hi << (32 - 8 * sh));
                } else word = g[0] | (uint32_t)g[1] << 8 | (uint32_t)g[2] << 16 | (uint32_t)g[3] << 24;
            } else
                for (int t = 0; t < 4; ++t) {
                    const int h = h0 + t;
                    if (h >= 3 * hw) break;
                    const int px = h / 3, c = h - 3 * px;
                    int sx = X0 + px;
                    if (sx < 0 || sx >= W) { if (!reflect) continue; sx = ss_redact_reflect(sx, W); }
                    word |= (uint32_t)rowp[(size_t)sx * 3 + c] << (8 * t);
                }
        }
        *reinterpret_cast<uint32_t*>(raw + j * pitch + h0) = word;
    }
}

// LDS of k_redact_compute at the call's effect and strength (dynamic, below 64 KiB: 62 104 bytes at r = 31)
static int rd_lds_bytes(int effect, int strength)
{
    if (effect == RD_BLUR) {
        const int hw = RD_TW + 2 * strength, hh = RD_TH + 2 * strength, pitch = (3 * hw + 3) & ~3;
        return RD_HEAD + hh * pitch + RD_TH * pitch * 2;
    }
    if (effect == RD_PIXELATE) return RD_HEAD + RD_TH * RD_TW * 3 + RD_TH * 16 * 3 * 4 + 8 * 16 * 3 + 128;
    return RD_HEAD;
}

__global__ __launch_bounds__(256) void k_redact_compute(const uint8_t* __restrict__ frames, long long frame_stride, int H, int W, int rs,
                                                        const RdRegion* __restrict__ regs, const int* __restrict__ reg_off, const int* __restrict__ verts,
                                                        int tx, int tiles, int effect, int strength, unsigned magic, int fill,
                                                        const int* __restrict__ count, const unsigned* __restrict__ list, uint8_t* __restrict__ slots)
{
    extern __shared__ __attribute__((aligned(16))) uint8_t lds[];
    unsigned short* hits = reinterpret_cast<unsigned short*>(lds);
    int* nhit = reinterpret_cast<int*>(lds + 2048);
    uint8_t* raw = lds + RD_HEAD;
    const int tid = threadIdx.x, y = tid >> 3, sg = tid & 7;
    const int n = *count;
    for (int it = blockIdx.x; it < n; it += gridDim.x) {
        const unsigned id = list[it];
        const int b = (int)(id / (unsigned)tiles), t = (int)(id % (unsigned)tiles), X = (t % tx) * RD_TW, Y = (t / tx) * RD_TH;
        const uint8_t* frame = frames + (size_t)b * frame_stride;
        const int r0 = reg_off[b], r1 = min(reg_off[b + 1], r0 + RD_MAXREG);
        __syncthreads();                                             // the tile before is done with the LDS
        if (tid == 0) *nhit = 0;
        __syncthreads();
        for (int i = r0 + tid; i < r1; i += 256)
            if (rd_meets(regs[i], H, W, X, Y)) hits[atomicAdd(nhit, 1)] = (unsigned short)(i - r0);
        uint32_t out[6] = {0, 0, 0, 0, 0, 0};                        // this thread's 8 pixels, 24 bytes
        if (effect == RD_BLUR) {
            const int r = strength, hw = RD_TW + 2 * r, hh = RD_TH + 2 * r, pitch = (3 * hw + 3) & ~3;
            unsigned short* vs = reinterpret_cast<unsigned short*>(raw + hh * pitch);     // column sums [32][pitch]
            rd_load(raw, pitch, frame, H, W, rs, X - r, Y - r, hw, hh, true, tid);
            __syncthreads();
            // column sums running down the rows, four byte columns (one LDS word) and 16 output rows a thread
            for (int i = tid; i < (pitch >> 2) * 2; i += 256) {
                const int g = i >> 1, y0 = (i & 1) * (RD_TH / 2);
                const uint32_t* col = reinterpret_cast<const uint32_t*>(raw) + g;
                const int wp = pitch >> 2;
                int s0 = 0, s1 = 0, s2 = 0, s3 = 0;
                for (int j = y0; j <= y0 + 2 * r; ++j) { const uint32_t v = col[j * wp]; s0 += v & 255; s1 += (v >> 8) & 255; s2 += (v >> 16) & 255; s3 += v >> 24; }
                for (int yy = y0;; ++yy) {
                    uint32_t* o = reinterpret_cast<uint32_t*>(vs + yy * pitch + 4 * g);
                    o[0] = (uint32_t)s0 | (uint32_t)s1 << 16; o[1] = (uint32_t)s2 | (uint32_t)s3 << 16;
                    if (yy == y0 + RD_TH / 2 - 1) break;
                    const uint32_t in = col[(yy + 2 * r + 1) * wp], out_ = col[yy * wp];
                    s0 += (int)(in & 255) - (int)(out_ & 255); s1 += (int)((in >> 8) & 255) - (int)((out_ >> 8) & 255);
                    s2 += (int)((in >> 16) & 255) - (int)((out_ >> 16) & 255); s3 += (int)(in >> 24) - (int)(out_ >> 24);
                }
            }
            __syncthreads();
            const unsigned d = (unsigned)((2 * r + 1) * (2 * r + 1));
            const unsigned short* row = vs + y * pitch + 8 * sg * 3;
            // the window of the thread's first pixel: 3 (2r + 1) consecutive u16, B G R B G R ..., two pixels (three words) a step
            const uint32_t* rw = reinterpret_cast<const uint32_t*>(row);
            int s[3] = {0, 0, 0};
            for (int i = 0; i < r; ++i) {
                const uint32_t d0 = rw[3 * i], d1 = rw[3 * i + 1], d2 = rw[3 * i + 2];
                s[0] += (int)(d0 & 0xffff) + (int)(d1 >> 16); s[1] += (int)(d0 >> 16) + (int)(d2 & 0xffff); s[2] += (int)(d1 & 0xffff) + (int)(d2 >> 16);
            }
            { const uint32_t d0 = rw[3 * r], d1 = rw[3 * r + 1]; s[0] += (int)(d0 & 0xffff); s[1] += (int)(d0 >> 16); s[2] += (int)(d1 & 0xffff); }
#pragma unroll
            for (int p = 0; p < 8; ++p)
#pragma unroll
                for (int c = 0; c < 3; ++c) {
                    if (p) s[c] += row[(p + 2 * r) * 3 + c] - row[(p - 1) * 3 + c];
                    const int at = p * 3 + c;
                    out[at >> 2] |= ss_redact_mean((unsigned)s[c], d, magic) << (8 * (at & 3));
                }
        } else if (effect == RD_PIXELATE) {
            const int cs = strength, ncx = RD_TW / cs, ncy = RD_TH / cs, pitch = RD_TW * 3;
            int* part = reinterpret_cast<int*>(raw + RD_TH * pitch);
            uint8_t* cell = reinterpret_cast<uint8_t*>(part + RD_TH * 16 * 3);
            rd_load(raw, pitch, frame, H, W, rs, X, Y, RD_TW, RD_TH, false, tid);
            __syncthreads();
            for (int i = tid; i < RD_TH * ncx * 3; i += 256) {       // per row, the sum of each cell's pixels (zeros outside the frame)
                const int ch = i % 3, cx = (i / 3) % ncx, yy = i / (3 * ncx);
                const uint8_t* p0 = raw + yy * pitch + cx * cs * 3 + ch;
                int s = 0;
                for (int p = 0; p < cs; ++p) s += p0[p * 3];
                part[i] = s;
            }
            __syncthreads();
            for (int i = tid; i < ncy * ncx * 3; i += 256) {
                const int ch = i % 3, cx = (i / 3) % ncx, cy = i / (3 * ncx);
                int s = 0;
                for (int p = 0; p < cs; ++p) s += part[((cy * cs + p) * ncx + cx) * 3 + ch];
                const int nw = min(cs, W - (X + cx * cs)), nh = min(cs, H - (Y + cy * cs)), np = nw > 0 && nh > 0 ? nw * nh : 0;
                cell[i] = np ? (uint8_t)((s + np / 2) / np) : 0;
            }
            __syncthreads();
#pragma unroll
            for (int p = 0; p < 8; ++p) {
                const uint8_t* cv = cell + ((y / cs) * ncx + (8 * sg + p) / cs) * 3;
#pragma unroll
                for (int c = 0; c < 3; ++c) { const int at = p * 3 + c; out[at >> 2] |= (uint32_t)cv[c] << (8 * (at & 3)); }
            }
        } else {
#pragma unroll
            for (int p = 0; p < 8; ++p)
#pragma unroll
                for (int c = 0; c < 3; ++c) { const int at = p * 3 + c; out[at >> 2] |= (uint32_t)((fill >> (8 * c)) & 255) << (8 * (at & 3)); }
            __syncthreads();                                         // the sublist is complete
        }
        const int nh_ = *nhit;
        unsigned mask = 0;
        const int py = Y + y;
        unsigned live = 0;                                           // the thread's pixels that lie in the frame
        if (py < H)
            for (int p = 0; p < 8; ++p) live |= (unsigned)(X + 8 * sg + p < W) << p;
        for (int h = 0; h < nh_ && mask != live; ++h) {              // one region at a time over the eight pixels
            const RdRegion g = regs[r0 + hits[h]];
            for (int p = 0; p < 8; ++p)
                if ((live & ~mask) >> p & 1) mask |= (unsigned)rd_covers(g, X + 8 * sg + p, py, H, W, verts) << p;
        }
        uint8_t* slot = slots + (size_t)it * RD_SLOT;
        uint2* dst = reinterpret_cast<uint2*>(slot + y * (RD_TW * 3) + sg * 24);
        dst[0] = make_uint2(out[0], out[1]); dst[1] = make_uint2(out[2], out[3]); dst[2] = make_uint2(out[4], out[5]);
        slot[RD_PIX + tid] = (uint8_t)mask;
    }
}

__global__ __launch_bounds__(256) void k_redact_store(uint8_t* __restrict__ frames, long long frame_stride, int rs, int tx, int tiles,
                                                      const int* __restrict__ count, const unsigned* __restrict__ list, const uint8_t* __restrict__ slots)
{
    const int tid = threadIdx.x, y = tid >> 3, sg = tid & 7;
    const int n = *count;
    for (int it = blockIdx.x; it < n; it += gridDim.x) {
        const uint8_t* slot = slots + (size_t)it * RD_SLOT;
        const unsigned mask = slot[RD_PIX + tid];
        if (!mask) continue;
        const unsigned id = list[it];
        const int b = (int)(id / (unsigned)tiles), t = (int)(id % (unsigned)tiles), X = (t % tx) * RD_TW, Y = (t / tx) * RD_TH;
        const uint8_t* src = slot + y * (RD_TW * 3) + sg * 24;
        uint8_t* dst = frames + (size_t)b * frame_stride + (size_t)(Y + y) * rs + (size_t)(X + 8 * sg) * 3;
        if (mask == 255u && ((uintptr_t)dst & 3) == 0) {            // all eight covered and the 24 bytes word-aligned in the frame
            const uint2* s2 = reinterpret_cast<const uint2*>(src);
            const uint2 a = s2[0], b2 = s2[1], c = s2[2];
            uint32_t* d4 = reinterpret_cast<uint32_t*>(dst);
            d4[0] = a.x; d4[1] = a.y; d4[2] = b2.x; d4[3] = b2.y; d4[4] = c.x; d4[5] = c.y;
            continue;
        }
        for (int p = 0; p < 8; ++p)
            if (mask >> p & 1) { dst[3 * p] = src[3 * p]; dst[3 * p + 1] = src[3 * p + 1]; dst[3 * p + 2] = src[3 * p + 2]; }
    }
}

// ---- host ---------------------------------------------------------------------------------------------------------------
int ss_redact_max_regions_impl() { return RD_MAXREG; }
int ss_redact_max_vertices_impl() { return RD_MAXV; }
int ss_redact_max_radius_impl() { return SS_REDACT_MAX_RADIUS; }

long long ss_redact_scratch_bytes_impl(int batch, int h, int w)
{
    if (batch < 1 || batch > 65535 || h < 1 || w < 1 || h > RD_MAXSIDE || w > RD_MAXSIDE) return SS_ERR_INVALID;
    const long long n = (long long)batch * ((w + RD_TW - 1) / RD_TW) * ((h + RD_TH - 1) / RD_TH);
    return RD_LIST_AT + ((4 * n + 255) & ~255LL) + n * RD_SLOT;
}

int ss_redact_check_impl(const uint8_t* d_frames, int batch, long long frame_batch_stride, int h, int w, int row_stride, const int* d_regions,
                         const int* d_region_off, const int* d_verts, int effect, int strength, int fill_bgr, const void* d_scratch,
                         long long scratch_bytes, std::string& err)
{
    const std::string who = "ss_redact: ";
    std::string bad;
    if (!d_frames || !d_regions || !d_region_off || !d_verts || !d_scratch) bad = "null pointer";
    else if (batch < 1 || batch > 65535) bad = "batch outside 1..65535";
    else if (h < 1 || w < 1 || h > RD_MAXSIDE || w > RD_MAXSIDE) bad = "frame size outside 1..8192";
    else if (row_stride < 3 * w) bad = "row_stride below 3 * w";
    else if (batch > 1 && frame_batch_stride < (long long)h * row_stride) bad = "frames overlap (frame_batch_stride below h * row_stride)";
    else if (effect < RD_BLUR || effect > RD_FILL) bad = "effect outside 0..2 (blur, pixelate, fill)";
    else if (effect == RD_BLUR && (strength < 1 || strength > SS_REDACT_MAX_RADIUS)) bad = "blur radius outside 1..31";
    else if (effect == RD_PIXELATE && strength != 4 && strength != 8 && strength != 16 && strength != 32) bad = "pixelate cell not one of 4, 8, 16, 32";
    else if (fill_bgr < 0 || fill_bgr > 0xffffff) bad = "fill colour outside 0..0xffffff";
    else if (((uintptr_t)d_scratch & 15) != 0) bad = "scratch not 16-byte aligned";
    else if (scratch_bytes < ss_redact_scratch_bytes_impl(batch, h, w))
        bad = "scratch_bytes " + std::to_string(scratch_bytes) + " is below ss_redact_scratch_bytes = " + std::to_string(ss_redact_scratch_bytes_impl(batch, h, w));
    if (!bad.empty()) { err = who + bad; return SS_ERR_INVALID; }
    return SS_OK;
}

int ss_redact_impl(hipStream_t st, uint8_t* d_frames, int batch, long long frame_batch_stride, int h, int w, int row_stride, const int* d_regions,
                   const int* d_region_off, const int* d_verts, int effect, int strength, int fill_bgr, void* d_scratch, std::string& err)
{
    const std::string who = "ss_redact: ";
    const int tx = (w + RD_TW - 1) / RD_TW, tiles = tx * ((h + RD_TH - 1) / RD_TH), total = batch * tiles;
    uint8_t* base = static_cast<uint8_t*>(d_scratch);
    int* count = reinterpret_cast<int*>(base);
    unsigned* list = reinterpret_cast<unsigned*>(base + RD_LIST_AT);
    uint8_t* slots = base + RD_LIST_AT + ((4LL * total + 255) & ~255LL);
    const RdRegion* regs = reinterpret_cast<const RdRegion*>(d_regions);
    SS_HIPCHK(who, hipMemsetAsync(count, 0, sizeof(int), st));
    hipLaunchKernelGGL(k_redact_tiles, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, st, regs, d_region_off, total, h, w, tx, tiles, count, list);
    const unsigned magic = effect == RD_BLUR ? ss_redact_div_magic(strength) : 0u;
    hipLaunchKernelGGL(k_redact_compute, dim3((unsigned)(total < 1024 ? total : 1024)), dim3(256), (size_t)rd_lds_bytes(effect, strength), st, d_frames,
                       frame_batch_stride, h, w, row_stride, regs, d_region_off, d_verts, tx, tiles, effect, strength, magic, fill_bgr, count, list, slots);
    hipLaunchKernelGGL(k_redact_store, dim3((unsigned)(total < 2048 ? total : 2048)), dim3(256), 0, st, d_frames, frame_batch_stride, row_stride, tx, tiles,
                       count, list, slots);
    SS_HIPCHK(who, hipGetLastError());
    return SS_OK;
}
