// ss_zone.hip — analytics behind the trackers (docs/ZONES.md): line crossings, zone occupancy and dwell, a cumulative heat map, and the
// blend of that heat map over resident BGR frames.  It reads the rows every tracker leaves on the device
// ([n_frames][n_streams][SS_MAXT][8] and their counts) and changes nothing upstream.  tests/zones_ref.py is the definition.
//
// k_zone_update: one launch per group, one workgroup per stream, the frames strictly in order, one thread per row.  The stream's
// live tracks (id, last frame, last anchor, inside bits, entry frame per zone) sit in a 1024-slot open-addressed table that is
// loaded into LDS once (92 KiB of the CU's 160), walked for every frame of the group and stored back.  A frame runs in five
// steps between barriers: (1) every row finds its id (read only) and rows of one id settle on the lowest by an LDS atomicMin,
// (2) thread 0 inserts the ids that were not found, in row order, so which rows share an id or find no slot does not depend on
// timing, (3) every counted row does its own f64 tests and updates its own slot; totals are LDS integer atomics, (4) the heat
// adds (integer atomics on the stream's grid in HBM: order-free, so exact), (5) the per-frame outputs.  An entry not seen for more
// than max_gap frames is expired: a lookup walks past it, an insert reuses it, and at the start of every launch the expired
// entries from which only expired entries lead to an empty slot are emptied (no probe chain of a live entry passes through them).
//
// k_zone_heat_blend: memory bound, in place, 16-byte accesses on the aligned body of every row,
// the bytes before and after it one by one; integer arithmetic only, so the NumPy formula reproduces every byte.
#include <cstddef>
#include <cstdint>
#include <cstring>
#include <vector>
#include "ss_common.h"
#include "ss_host.h"
#include "ss_launch.h"

#define ZN_LINES 16
#define ZN_ZONES 16
#define ZN_VERTS 32
#define ZN_LIVE 1024                   // slots of a stream's table = the most live tracks
#define ZN_CELLS 65536                 // the most heat cells of a stream
#define ZN_FREE 0x7fffffff             // claim word of a slot no row of the frame has found
#define ZN_NOSLOT (-1)
#define ZN_DUP (-2)

struct ZnTable {                       // one stream's live tracks; id 0: the slot is empty
    double ax[ZN_LIVE], ay[ZN_LIVE];   // last anchor, doubled coordinates
    int id[ZN_LIVE], last[ZN_LIVE];    // last: the stream's frame index of the last appearance
    unsigned inside[ZN_LIVE];
    int entry[ZN_LIVE][ZN_ZONES];      // frame of the entry into each zone the track is inside
};
struct ZnGeom {                        // doubled coordinates
    double line[ZN_LINES][4];          // ax, ay, bx, by
    double poly[ZN_ZONES][ZN_VERTS][2];
    int nv[ZN_ZONES];
};
struct ZnTot {                         // one stream's running totals
    long long dwell_sum[ZN_ZONES];
    int line[ZN_LINES][2];             // in, out
    int entries[ZN_ZONES], exits[ZN_ZONES], longest[ZN_ZONES], peak[ZN_ZONES];
    int frame, heat_max, pad[2];
};
static_assert(sizeof(ZnTable) % 16 == 0 && sizeof(ZnGeom) % 16 == 0 && sizeof(ZnTot) % 16 == 0, "copied in 16-byte pieces");

struct SSZoneDev {
    int S, n_lines, n_zones, anchor, max_gap, n_classes, heat, k, h, w, gh, gw;
    ZnTable* table;                    // [S]
    ZnGeom* geom;
    ZnTot* tot;                        // [S]
    int* line_class;                   // [S][16][2][n_classes]
    int* grid;                         // [S][gh][gw]
    int* err;                          // [S]
    uint32_t* lut;                     // [256] B | G << 8 | R << 16
};

struct ZnLds {
    ZnTable t;
    ZnGeom g;
    ZnTot tot;
    int claim[ZN_LIVE];                // lowest row of the frame that found the slot
    int occ[ZN_ZONES];
    int rslot[SS_MAXT];                // what thread 0 settled for a row whose id was not found
    int nid[SS_MAXT];
    int rect[SS_MAXT][4];              // heat "box": cells cx0, cx1, cy0, cy1 (cx0 > cx1: none)
    unsigned long long newmask[SS_MAXT / 64];
};

__device__ __forceinline__ void zn_copy16(void* dst, const void* src, int bytes)
{
    for (int i = threadIdx.x * 16; i < bytes; i += blockDim.x * 16)
        *reinterpret_cast<uint4*>((char*)dst + i) = *reinterpret_cast<const uint4*>((const char*)src + i);
}

__global__ __launch_bounds__(256) void k_zone_update(SSZoneDev z, int F, const float* __restrict__ rows, const int* __restrict__ nrows,
                                                     uint32_t* __restrict__ events, uint32_t* __restrict__ inside, int* __restrict__ dwell,
                                                     int* __restrict__ line_totals, int* __restrict__ occupancy, int* __restrict__ heat_frames,
                                                     int* __restrict__ heat_max)
{
    __shared__ __attribute__((aligned(16))) ZnLds m;
    const int s = blockIdx.x, tid = threadIdx.x, S = z.S;
    // a stream that takes part in no frame of the group (every count negative) keeps its state where it is
    if (!__syncthreads_or(tid < F && nrows[tid * S + s] >= 0)) return;
    const int table_bytes = z.n_zones ? (int)sizeof(ZnTable) : (int)offsetof(ZnTable, entry);
    zn_copy16(&m.t, z.table + s, table_bytes);
    zn_copy16(&m.g, z.geom, sizeof(ZnGeom));
    zn_copy16(&m.tot, z.tot + s, sizeof(ZnTot));
    if (tid < ZN_ZONES) m.occ[tid] = 0;
    __syncthreads();
    int f = m.tot.frame;
    const int gap = z.max_gap;
    // expired entries behind which only expired entries lead to an empty slot: emptied
    for (int t = tid; t < ZN_LIVE; t += blockDim.x) {
        int can = 0;
        if (m.t.id[t] != 0 && f - m.t.last[t] > gap)
            for (int k = 1, u = t; k < ZN_LIVE; ++k) {
                u = (u + 1) & (ZN_LIVE - 1);
                if (m.t.id[u] == 0) { can = 1; break; }
                if (f - m.t.last[u] <= gap) break;
            }
        m.claim[t] = can;
    }
    __syncthreads();
    for (int t = tid; t < ZN_LIVE; t += blockDim.x) {
        if (m.claim[t]) m.t.id[t] = 0;
        m.claim[t] = ZN_FREE;
    }
    __syncthreads();

    int* grid = z.grid + (size_t)s * z.gh * z.gw;
    for (int fi = 0; fi < F; ++fi) {
        int n = nrows[fi * S + s];
        if (n < 0) continue;                                     // uniform: the stream sits this frame out
        n = min(n, SS_MAXT);
        const size_t fs = (size_t)fi * S + s;
        const int r = tid;
        // ---- (1) the row, its id, its slot
        float4 bx = make_float4(0.f, 0.f, 0.f, 0.f), mt = bx;
        if (r < n) {
            const float4* p = reinterpret_cast<const float4*>(rows + (fs * SS_MAXT + r) * 8);
            bx = p[0]; mt = p[1];
        }
        const bool valid = r < n && mt.x >= 1.0f && mt.x < 2147483648.0f && __builtin_isfinite(bx.x) && __builtin_isfinite(bx.y) &&
                           __builtin_isfinite(bx.z) && __builtin_isfinite(bx.w);
        const int id = valid ? (int)mt.x : 0;
        int slot = ZN_NOSLOT;
        bool found = false;
        if (valid) {
            for (int k = 0, t = id & (ZN_LIVE - 1); k < ZN_LIVE; ++k, t = (t + 1) & (ZN_LIVE - 1)) {
                const int e = m.t.id[t];
                if (e == 0) break;
                if (e == id) { if (f - m.t.last[t] <= gap) { slot = t; found = true; } break; }
            }
            if (found) atomicMin(&m.claim[slot], r);
        }
        const bool isnew = valid && !found;
        m.nid[r] = id;
        const unsigned long long bm = __ballot(isnew);
        if ((tid & 63) == 0) m.newmask[tid >> 6] = bm;
        __syncthreads();
        // ---- (2) the ids that were not found, in row order
        if (tid == 0) {
            for (int wv = 0; wv < SS_MAXT / 64; ++wv) {
                unsigned long long mask = m.newmask[wv];
                while (mask) {
                    const int r2 = wv * 64 + __ffsll((long long)mask) - 1;
                    mask &= mask - 1;
                    const int id2 = m.nid[r2];
                    int res = ZN_NOSLOT, reuse = -1;
                    for (int k = 0, t = id2 & (ZN_LIVE - 1); k < ZN_LIVE; ++k, t = (t + 1) & (ZN_LIVE - 1)) {
                        const int e = m.t.id[t];
                        if (e == 0) { if (reuse < 0) reuse = t; break; }
                        const bool expired = f - m.t.last[t] > gap;
                        if (e == id2) {
                            if (!expired) res = ZN_DUP;          // a lower row of this frame brought the id in
                            else if (reuse < 0) reuse = t;
                            break;
                        }
                        if (expired && reuse < 0) reuse = t;
                    }
                    if (res != ZN_DUP) {
                        if (reuse >= 0) { m.t.id[reuse] = id2; m.t.last[reuse] = f; res = reuse; }
                        else z.err[s] = SS_ERR_CAPACITY;         // ZN_LIVE live tracks: the row counts as a first appearance and leaves no state
                    }
                    m.rslot[r2] = res;
                }
            }
        }
        __syncthreads();
        // ---- (3) every counted row: crossings, zones, its slot
        bool counted = valid;
        if (valid) {
            if (found) counted = m.claim[slot] == r;
            else { slot = m.rslot[r]; counted = slot != ZN_DUP; }
        }
        unsigned ev = 0, cur = 0;
        int dw = 0;
        int rc0 = 0, rc1 = -1, rc2 = 0, rc3 = -1;
        if (counted) {
            const double AX = (double)bx.x + (double)bx.z;
            const double AY = z.anchor ? 2.0 * (double)bx.w : (double)bx.y + (double)bx.w;
            const bool first = !found;
            if (!first) {
                const double P0x = m.t.ax[slot], P0y = m.t.ay[slot];
                const double dx = AX - P0x, dy = AY - P0y;
                for (int l = 0; l < z.n_lines; ++l) {
                    const double ax = m.g.line[l][0], ay = m.g.line[l][1], qx = m.g.line[l][2], qy = m.g.line[l][3];
                    const double ex = qx - ax, ey = qy - ay;
                    const double s0 = ex * (P0y - ay) - ey * (P0x - ax);
                    const double s1 = ex * (AY - ay) - ey * (AX - ax);
                    if ((s0 >= 0.0) != (s1 >= 0.0)) {
                        const double sa = dx * (ay - P0y) - dy * (ax - P0x);
                        const double sb = dx * (qy - P0y) - dy * (qx - P0x);
                        if ((sa >= 0.0) != (sb >= 0.0)) ev |= (s1 >= 0.0) ? (1u << l) : (1u << (16 + l));
                    }
                }
            }
            for (int zz = 0; zz < z.n_zones; ++zz) {
                const int nv = m.g.nv[zz];
                int par = 0;
                double vix = m.g.poly[zz][0][0], viy = m.g.poly[zz][0][1];
                for (int i = 0; i < nv; ++i) {
                    const int j = i + 1 == nv ? 0 : i + 1;
                    const double vjx = m.g.poly[zz][j][0], vjy = m.g.poly[zz][j][1];
                    if ((viy > AY) != (vjy > AY)) {
                        const double t = (vjx - vix) * (AY - viy) - (AX - vix) * (vjy - viy);
                        par ^= (vjy > viy) ? (t > 0.0) : (t < 0.0);
                    }
                    vix = vjx; viy = vjy;
                }
                cur |= (unsigned)par << zz;
            }
            if (ev) {
                const bool cls_ok = mt.y >= 0.0f && mt.y < (float)z.n_classes;
                const int cls = cls_ok ? (int)mt.y : 0;
                for (int l = 0; l < z.n_lines; ++l)
                    for (int d = 0; d < 2; ++d)
                        if (ev >> (16 * d + l) & 1u) {
                            atomicAdd(&m.tot.line[l][d], 1);
                            if (cls_ok) atomicAdd(&z.line_class[(((size_t)s * ZN_LINES + l) * 2 + d) * z.n_classes + cls], 1);
                        }
            }
            const unsigned prev = first ? 0u : m.t.inside[slot];
            const int last = first ? f : m.t.last[slot];
            for (int zz = 0; zz < z.n_zones; ++zz) {
                const unsigned bit = 1u << zz;
                if (prev & ~cur & bit) {                         // exit: the stay ended with the previous appearance
                    const int d = last - m.t.entry[slot][zz] + 1;
                    atomicAdd(&m.tot.exits[zz], 1);
                    atomicAdd(reinterpret_cast<unsigned long long*>(&m.tot.dwell_sum[zz]), (unsigned long long)d);
                    atomicMax(&m.tot.longest[zz], d);
                }
                if (cur & bit) {
                    int e = f;
                    if (prev & bit) e = m.t.entry[slot][zz];
                    else { atomicAdd(&m.tot.entries[zz], 1); if (slot >= 0) m.t.entry[slot][zz] = f; }
                    dw = max(dw, f - e + 1);
                    atomicAdd(&m.occ[zz], 1);
                }
            }
            if (slot >= 0) { m.t.ax[slot] = AX; m.t.ay[slot] = AY; m.t.last[slot] = f; m.t.inside[slot] = cur; }
            if (z.heat == 1) {
                const double px = floor(AX * 0.5), py = floor(AY * 0.5);
                if (px >= 0.0 && px < (double)z.w && py >= 0.0 && py < (double)z.h) {
                    const int old = atomicAdd(&grid[((int)py >> z.k) * z.gw + ((int)px >> z.k)], 1);
                    atomicMax(&m.tot.heat_max, old + 1);
                }
            } else if (z.heat == 2) {
                const double x0 = fmax(floor((double)bx.x), 0.0), x1 = fmin(ceil((double)bx.z) - 1.0, (double)(z.w - 1));
                const double y0 = fmax(floor((double)bx.y), 0.0), y1 = fmin(ceil((double)bx.w) - 1.0, (double)(z.h - 1));
                if (x0 <= x1 && y0 <= y1) { rc0 = (int)x0 >> z.k; rc1 = (int)x1 >> z.k; rc2 = (int)y0 >> z.k; rc3 = (int)y1 >> z.k; }
            }
        }
        if (z.heat == 2) { m.rect[r][0] = rc0; m.rect[r][1] = rc1; m.rect[r][2] = rc2; m.rect[r][3] = rc3; }
        if (events) events[fs * SS_MAXT + r] = ev;
        if (inside) inside[fs * SS_MAXT + r] = cur;
        if (dwell) dwell[fs * SS_MAXT + r] = dw;
        __syncthreads();
        // ---- (4) heat of the boxes: all threads over each row's cells; the claims of this frame are given back
        if (counted && found) m.claim[slot] = ZN_FREE;
        if (z.heat == 2) {
            int lmax = 0;
            for (int r2 = 0; r2 < n; ++r2) {
                const int cx0 = m.rect[r2][0], ncx = m.rect[r2][1] - cx0 + 1, cy0 = m.rect[r2][2], ncy = m.rect[r2][3] - cy0 + 1;
                if (ncx <= 0 || ncy <= 0) continue;
                for (int i = tid; i < ncx * ncy; i += blockDim.x) {
                    const int cy = i / ncx, cx = i - cy * ncx;
                    lmax = max(lmax, atomicAdd(&grid[(cy0 + cy) * z.gw + cx0 + cx], 1) + 1);
                }
            }
            if (lmax) atomicMax(&m.tot.heat_max, lmax);
        }
        if (z.heat && heat_frames) __threadfence();              // the adds have arrived before the grid is read back below
        __syncthreads();
        // ---- (5) what the frame leaves behind
        if (tid < 2 * ZN_LINES && line_totals) line_totals[fs * 2 * ZN_LINES + tid] = (&m.tot.line[0][0])[tid];
        if (tid < ZN_ZONES) {
            const int o = m.occ[tid];
            if (occupancy) occupancy[fs * ZN_ZONES + tid] = o;
            m.tot.peak[tid] = max(m.tot.peak[tid], o);
            m.occ[tid] = 0;
        }
        if (z.heat && heat_frames) {
            int* dst = heat_frames + fs * z.gh * z.gw;
            for (int i = tid; i < z.gh * z.gw; i += blockDim.x) dst[i] = __hip_atomic_load(&grid[i], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        }
        if (tid == 0 && heat_max) heat_max[fs] = m.tot.heat_max;
        ++f;
    }
    __syncthreads();
    if (tid == 0) m.tot.frame = f;
    __syncthreads();
    zn_copy16(z.table + s, &m.t, table_bytes);
    zn_copy16(z.tot + s, &m.tot, sizeof(ZnTot));
}

// ---- heat blend ---------------------------------------------------------------------------------------------------
// colour of pixel x of a row whose heat cells are hrow (0 in bit 31: the pixel stays as it is)
__device__ __forceinline__ uint32_t zn_colour(const int* __restrict__ hrow, int cx, unsigned mm, const uint32_t* __restrict__ lut)
{
    const int v = hrow[cx];
    if (v <= 0) return 0x80000000u;
    const unsigned vv = min((unsigned)v, mm);
    const unsigned t = mm <= 0x800000u ? (vv * 255u + (mm >> 1)) / mm : (unsigned)(((unsigned long long)vv * 255u + (mm >> 1)) / mm);
    return lut[t];
}

__device__ __forceinline__ unsigned zn_mix(unsigned pix, unsigned col, unsigned a) { return (pix * (256u - a) + col * a + 128u) >> 8; }

// one frame row: where it starts, its heat cells, its frame's maximum, the bytes before its first 16-byte boundary and its 16-byte pieces
struct ZnRow { uint8_t* row; const int* hrow; unsigned mm; int hb, nb; };

__device__ __forceinline__ ZnRow zn_row(long long ry, uint8_t* frames, long long frame_stride, int h, int nbytes, int row_stride, const int* heat,
                                        long long heat_stride, const int* maxes, int max_stride, int k, int gw)
{
    ZnRow r;
    const int b = (int)(ry / h), y = (int)(ry - (long long)b * h);
    r.row = frames + b * frame_stride + (long long)y * row_stride;
    r.hrow = heat + b * heat_stride + (long long)(y >> k) * gw;
    r.mm = (unsigned)max(maxes[(long long)b * max_stride], 1);
    r.hb = min((int)((16 - ((uintptr_t)r.row & 15)) & 15), nbytes);
    r.nb = (nbytes - r.hb) >> 4;
    return r;
}

// the 16 bytes at offset o of a row, blended in registers; true when a byte changed
__device__ __forceinline__ bool zn_piece(unsigned (&wd)[4], int o, const ZnRow& r, int k, const uint32_t* __restrict__ lut, unsigned a)
{
    int x = o / 3, c = o - 3 * x, cell = -1;
    uint32_t col = 0x80000000u;
    bool dirty = false;
#pragma unroll
    for (int i = 0; i < 16; ++i) {
        if ((x >> k) != cell) { cell = x >> k; col = zn_colour(r.hrow, cell, r.mm, lut); }
        if (!(col >> 31)) {
            const int sh = 8 * (i & 3);
            const unsigned out = zn_mix((wd[i >> 2] >> sh) & 255u, (col >> (8 * c)) & 255u, a);
            wd[i >> 2] = (wd[i >> 2] & ~(255u << sh)) | (out << sh);
            dirty = true;
        }
        if (++c == 3) { c = 0; ++x; }
    }
    return dirty;
}

// the bytes before and after the aligned body, one by one
__device__ __forceinline__ void zn_edges(const ZnRow& r, int nbytes, int k, const uint32_t* __restrict__ lut, unsigned a)
{
    for (int part = 0; part < 2; ++part)
        for (int o = part ? r.hb + 16 * r.nb : 0; o < (part ? nbytes : r.hb); ++o) {
            const int x = o / 3, c = o - 3 * x;
            const uint32_t col = zn_colour(r.hrow, x >> k, r.mm, lut);
            if (!(col >> 31)) r.row[o] = (uint8_t)zn_mix(r.row[o], (col >> (8 * c)) & 255u, a);
        }
}

// One workgroup per row (grid-stride), one thread per 16-byte piece of its aligned body; the thread behind the last piece does the edges
__global__ __launch_bounds__(256) void k_zone_heat_blend(uint8_t* __restrict__ frames, int batch, long long frame_stride, int h, int w, int row_stride,
                                                         const int* __restrict__ heat, long long heat_stride, const int* __restrict__ maxes,
                                                         int max_stride, int k, int gw, const uint32_t* __restrict__ lut, unsigned a)
{
    const int nbytes = 3 * w;
    for (long long ry = blockIdx.x; ry < (long long)batch * h; ry += gridDim.x) {
        const ZnRow r = zn_row(ry, frames, frame_stride, h, nbytes, row_stride, heat, heat_stride, maxes, max_stride, k, gw);
        for (int j = threadIdx.x; j <= r.nb; j += blockDim.x) {
            if (j < r.nb) {
                uint4* p = reinterpret_cast<uint4*>(r.row + r.hb + 16 * j);
                const uint4 q = *p;
                unsigned wd[4] = {q.x, q.y, q.z, q.w};
                if (zn_piece(wd, r.hb + 16 * j, r, k, lut, a)) *p = make_uint4(wd[0], wd[1], wd[2], wd[3]);
            } else {
                zn_edges(r, nbytes, k, lut, a);
            }
        }
    }
}

// ---- host side ------------------------------------------------------------------------------------------------------
struct SSZone {
    SSZoneDev dev;
    ss_zone_config cfg;
    SsBuf<SS_DEVICE> table, geom, tot, line_class, grid, err, lut;
    bool has_lut = false;
};

int ss_zone_max_lines_impl() { return ZN_LINES; }
int ss_zone_max_zones_impl() { return ZN_ZONES; }
int ss_zone_max_vertices_impl() { return ZN_VERTS; }
int ss_zone_max_live_impl() { return ZN_LIVE; }

void ss_zone_free(SSZone* z) { delete z; }

int ss_zone_create_check_impl(const ss_zone_config* cfg, const int* lines, int n_lines, const int* poly_xy, const int* poly_off, int n_zones,
                              std::string& err)
{
    const std::string who = "ss_zone_create: ";
    if (!cfg) { err = who + "null configuration"; return SS_ERR_INVALID; }
    if (cfg->anchor != 0 && cfg->anchor != 1) { err = who + "anchor must be 0 (centre) or 1 (bottom)"; return SS_ERR_INVALID; }
    if (cfg->max_gap < 1 || cfg->max_gap > 32) { err = who + "max_gap " + std::to_string(cfg->max_gap) + " outside 1..32"; return SS_ERR_INVALID; }
    if (cfg->n_classes < 1 || cfg->n_classes > 128) { err = who + "n_classes " + std::to_string(cfg->n_classes) + " outside 1..128"; return SS_ERR_INVALID; }
    if (cfg->heat < 0 || cfg->heat > 2) { err = who + "heat must be 0 (off), 1 (anchor) or 2 (box)"; return SS_ERR_INVALID; }
    if (cfg->heat_cell_log2 < 0 || cfg->heat_cell_log2 > 6) { err = who + "heat_cell_log2 " + std::to_string(cfg->heat_cell_log2) + " outside 0..6"; return SS_ERR_INVALID; }
    if (cfg->heat) {
        if (cfg->frame_h < 1 || cfg->frame_w < 1 || cfg->frame_h > 32768 || cfg->frame_w > 32768) { err = who + "heat needs a frame size of 1..32768 a side"; return SS_ERR_INVALID; }
        const int c = 1 << cfg->heat_cell_log2;
        const long long cells = (long long)((cfg->frame_h + c - 1) / c) * ((cfg->frame_w + c - 1) / c);
        if (cells > ZN_CELLS) { err = who + "heat grid of " + std::to_string(cells) + " cells is over the cap of " + std::to_string(ZN_CELLS); return SS_ERR_INVALID; }
    }
    if (n_lines < 0 || n_lines > ZN_LINES) { err = who + std::to_string(n_lines) + " lines, at most " + std::to_string(ZN_LINES); return SS_ERR_INVALID; }
    if (n_zones < 0 || n_zones > ZN_ZONES) { err = who + std::to_string(n_zones) + " zones, at most " + std::to_string(ZN_ZONES); return SS_ERR_INVALID; }
    if ((n_lines && !lines) || (n_zones && (!poly_xy || !poly_off))) { err = who + "null geometry"; return SS_ERR_INVALID; }
    for (int l = 0; l < n_lines; ++l) {
        for (int i = 0; i < 4; ++i)
            if (lines[4 * l + i] < -32767 || lines[4 * l + i] > 32767) { err = who + "line " + std::to_string(l) + ": coordinate " + std::to_string(lines[4 * l + i]) + " outside -32767..32767"; return SS_ERR_INVALID; }
        if (lines[4 * l] == lines[4 * l + 2] && lines[4 * l + 1] == lines[4 * l + 3]) { err = who + "line " + std::to_string(l) + ": both ends are the same point"; return SS_ERR_INVALID; }
    }
    if (n_zones && poly_off[0] != 0) { err = who + "poly_off[0] must be 0"; return SS_ERR_INVALID; }
    for (int q = 0; q < n_zones; ++q) {
        const long long nv = (long long)poly_off[q + 1] - poly_off[q];
        if (nv < 3 || nv > ZN_VERTS) { err = who + "zone " + std::to_string(q) + ": " + std::to_string(nv) + " vertices, 3 to " + std::to_string(ZN_VERTS) + " allowed"; return SS_ERR_INVALID; }
        for (int i = 2 * poly_off[q]; i < 2 * poly_off[q + 1]; ++i)
            if (poly_xy[i] < -32767 || poly_xy[i] > 32767) { err = who + "zone " + std::to_string(q) + ": coordinate " + std::to_string(poly_xy[i]) + " outside -32767..32767"; return SS_ERR_INVALID; }
    }
    return SS_OK;
}

int ss_zone_reset_impl(SSZone* z, hipStream_t st, int stream, std::string& err)
{
    const char* who = "ss_zone_reset: ";
    const SSZoneDev& d = z->dev;
    const size_t s0 = stream < 0 ? 0 : stream, ns = stream < 0 ? d.S : 1;
    SS_HIPCHK(who, hipMemsetAsync(d.table + s0, 0, ns * sizeof(ZnTable), st));
    SS_HIPCHK(who, hipMemsetAsync(d.tot + s0, 0, ns * sizeof(ZnTot), st));
    SS_HIPCHK(who, hipMemsetAsync(d.line_class + s0 * ZN_LINES * 2 * d.n_classes, 0, ns * ZN_LINES * 2 * d.n_classes * sizeof(int), st));
    SS_HIPCHK(who, hipMemsetAsync(d.grid + s0 * d.gh * d.gw, 0, ns * (size_t)d.gh * d.gw * sizeof(int), st));
    SS_HIPCHK(who, hipMemsetAsync(d.err + s0, 0, ns * sizeof(int), st));
    SS_HIPCHK(who, hipStreamSynchronize(st));
    return SS_OK;
}

int ss_zone_create_impl(SSZone** pz, hipStream_t st, int S, const ss_zone_config* cfg, const int* lines, int n_lines, const int* poly_xy,
                        const int* poly_off, int n_zones, std::string& err)
{
    const char* who = "ss_zone_create: ";
    SSZone* z = new SSZone();
    z->cfg = *cfg;
    SSZoneDev& d = z->dev;
    memset(&d, 0, sizeof d);
    d.S = S; d.n_lines = n_lines; d.n_zones = n_zones; d.anchor = cfg->anchor; d.max_gap = cfg->max_gap; d.n_classes = cfg->n_classes;
    d.heat = cfg->heat; d.k = cfg->heat_cell_log2; d.h = cfg->frame_h; d.w = cfg->frame_w;
    const int c = 1 << d.k;
    d.gh = cfg->heat ? (d.h + c - 1) / c : 1;
    d.gw = cfg->heat ? (d.w + c - 1) / c : 1;
    ZnGeom g;
    memset(&g, 0, sizeof g);
    for (int l = 0; l < n_lines; ++l)
        for (int i = 0; i < 4; ++i) g.line[l][i] = 2.0 * lines[4 * l + i];
    for (int q = 0; q < n_zones; ++q) {
        g.nv[q] = poly_off[q + 1] - poly_off[q];
        for (int i = 0; i < g.nv[q]; ++i)
            for (int a = 0; a < 2; ++a) g.poly[q][i][a] = 2.0 * poly_xy[2 * (poly_off[q] + i) + a];
    }
    hipError_t e = z->table.reserve((size_t)S * sizeof(ZnTable), SS_EXACT);
    if (e == hipSuccess) e = z->geom.reserve(sizeof(ZnGeom), SS_EXACT);
    if (e == hipSuccess) e = z->tot.reserve((size_t)S * sizeof(ZnTot), SS_EXACT);
    if (e == hipSuccess) e = z->line_class.reserve((size_t)S * ZN_LINES * 2 * d.n_classes * sizeof(int), SS_EXACT);
    if (e == hipSuccess) e = z->grid.reserve((size_t)S * d.gh * d.gw * sizeof(int), SS_EXACT);
    if (e == hipSuccess) e = z->err.reserve((size_t)S * sizeof(int), SS_EXACT);
    if (e == hipSuccess) e = z->lut.reserve(256 * sizeof(uint32_t), SS_EXACT);
    if (e != hipSuccess) { delete z; err = std::string(who) + hipGetErrorString(e); return SS_ERR_HIP; }
    d.table = z->table.as<ZnTable>(); d.geom = z->geom.as<ZnGeom>(); d.tot = z->tot.as<ZnTot>(); d.line_class = z->line_class.as<int>();
    d.grid = z->grid.as<int>(); d.err = z->err.as<int>(); d.lut = z->lut.as<uint32_t>();
    *pz = z;
    SS_HIPCHK(who, hipMemcpy(d.geom, &g, sizeof g, hipMemcpyHostToDevice));
    SS_HIPCHK(who, hipMemset(d.lut, 0, 256 * sizeof(uint32_t)));
    return ss_zone_reset_impl(z, st, -1, err);
}

int ss_zone_update_check_impl(int n_frames, const float* d_rows, const int* d_nrows, std::string& err)
{
    const std::string who = "ss_zone_update_group: ";
    if (n_frames < 1 || n_frames > SS_FMAX) { err = who + "n_frames " + std::to_string(n_frames) + " outside 1.." + std::to_string(SS_FMAX); return SS_ERR_INVALID; }
    if (!d_rows || !d_nrows) { err = who + "null rows or counts"; return SS_ERR_INVALID; }
    if ((uintptr_t)d_rows & 15) { err = who + "rows must be 16-byte aligned"; return SS_ERR_INVALID; }
    return SS_OK;
}

int ss_zone_update_impl(SSZone* z, hipStream_t st, int n_frames, const float* d_rows, const int* d_nrows, uint32_t* d_events, uint32_t* d_inside,
                        int* d_dwell, int* d_line_totals, int* d_occupancy, int* d_heat_frames, int* d_heat_max, std::string& err)
{
    hipLaunchKernelGGL(k_zone_update, dim3(z->dev.S), dim3(256), 0, st, z->dev, n_frames, d_rows, d_nrows, d_events, d_inside, d_dwell, d_line_totals,
                       d_occupancy, d_heat_frames, d_heat_max);
    SS_HIPCHK("ss_zone_update_group: ", hipGetLastError());
    return SS_OK;
}

// the capacity flags, for ss_check_errors: SS_OK, or the code of the first stream that has one
int ss_zone_pending_impl(SSZone* z, hipStream_t st, std::string& err)
{
    if (!z) return SS_OK;
    const char* who = "ss_check_errors: ";
    std::vector<int> e(z->dev.S);
    SS_HIPCHK(who, hipMemcpyAsync(e.data(), z->dev.err, e.size() * sizeof(int), hipMemcpyDeviceToHost, st));
    SS_HIPCHK(who, hipStreamSynchronize(st));
    for (size_t s = 0; s < e.size(); ++s)
        if (e[s]) { err = "zone analytics: more than " + std::to_string(ZN_LIVE) + " live tracks on stream " + std::to_string(s); return e[s]; }
    return SS_OK;
}

int ss_zone_get_totals_impl(SSZone* z, hipStream_t st, int stream, int* frames, int* line_class, int* line_totals, int* zone_entries, int* zone_exits,
                            long long* zone_dwell_sum, int* zone_longest, int* zone_peak, int* heat_max, std::string& err)
{
    const char* who = "ss_zone_get_totals: ";
    ZnTot t;
    SS_HIPCHK(who, hipStreamSynchronize(st));
    SS_HIPCHK(who, hipMemcpy(&t, z->dev.tot + stream, sizeof t, hipMemcpyDeviceToHost));
    const size_t lc = (size_t)ZN_LINES * 2 * z->dev.n_classes;
    if (line_class) SS_HIPCHK(who, hipMemcpy(line_class, z->dev.line_class + stream * lc, lc * sizeof(int), hipMemcpyDeviceToHost));
    if (frames) *frames = t.frame;
    if (heat_max) *heat_max = t.heat_max;
    if (line_totals) memcpy(line_totals, t.line, sizeof t.line);
    if (zone_entries) memcpy(zone_entries, t.entries, sizeof t.entries);
    if (zone_exits) memcpy(zone_exits, t.exits, sizeof t.exits);
    if (zone_dwell_sum) memcpy(zone_dwell_sum, t.dwell_sum, sizeof t.dwell_sum);
    if (zone_longest) memcpy(zone_longest, t.longest, sizeof t.longest);
    if (zone_peak) memcpy(zone_peak, t.peak, sizeof t.peak);
    return SS_OK;
}

int ss_zone_get_heat_impl(SSZone* z, hipStream_t st, int stream, int* grid, std::string& err)
{
    const char* who = "ss_zone_get_heat: ";
    const size_t cells = (size_t)z->dev.gh * z->dev.gw;
    SS_HIPCHK(who, hipStreamSynchronize(st));
    SS_HIPCHK(who, hipMemcpy(grid, z->dev.grid + stream * cells, cells * sizeof(int), hipMemcpyDeviceToHost));
    return SS_OK;
}

void ss_zone_shape_impl(const SSZone* z, int* S, int* heat, int* gh, int* gw, int* h, int* w)
{
    *S = z->dev.S; *heat = z->dev.heat; *gh = z->dev.gh; *gw = z->dev.gw; *h = z->dev.h; *w = z->dev.w;
}

void ss_zone_heat_device_impl(const SSZone* z, int stream, void** d_heat, void** d_max)
{
    *d_heat = z->dev.grid + (size_t)stream * z->dev.gh * z->dev.gw;
    *d_max = &z->dev.tot[stream].heat_max;
}

int ss_zone_set_colormap_impl(SSZone* z, const uint8_t* bgr, std::string& err)
{
    uint32_t lut[256];
    for (int i = 0; i < 256; ++i) lut[i] = bgr[3 * i] | (uint32_t)bgr[3 * i + 1] << 8 | (uint32_t)bgr[3 * i + 2] << 16;
    SS_HIPCHK("ss_zone_set_colormap: ", hipMemcpy(z->dev.lut, lut, sizeof lut, hipMemcpyHostToDevice));
    z->has_lut = true;
    return SS_OK;
}

int ss_zone_blend_check_impl(const uint8_t* d_frames, int batch, long long frame_batch_stride, int h, int w, int row_stride, const int* d_heat,
                             long long heat_frame_stride, const int* d_max, int max_stride, int alpha, std::string& err)
{
    const std::string who = "ss_zone_heat_blend: ";
    const char* bad = nullptr;
    if (!d_frames || !d_heat || !d_max) bad = "null pointer";
    else if (batch < 0 || batch > 65535) bad = "batch outside 0..65535";
    else if (h < 1 || w < 1 || h > 32768 || w > 32768) bad = "frame size outside 1..32768";
    else if (row_stride < 3 * w) bad = "row_stride below 3 * w";
    else if (batch > 1 && frame_batch_stride < (long long)h * row_stride) bad = "frames overlap (frame_batch_stride below h * row_stride)";
    else if (heat_frame_stride < 0 || max_stride < 0) bad = "negative heat or max stride";
    else if (alpha < 0 || alpha > 256) bad = "alpha outside 0..256";
    if (bad) { err = who + bad; return SS_ERR_INVALID; }
    return SS_OK;
}

int ss_zone_blend_impl(SSZone* z, hipStream_t st, uint8_t* d_frames, int batch, long long frame_batch_stride, int h, int w, int row_stride,
                       const int* d_heat, long long heat_frame_stride, const int* d_max, int max_stride, int alpha, std::string& err)
{
    const std::string who = "ss_zone_heat_blend: ";
    const SSZoneDev& d = z->dev;
    if (!d.heat) { err = who + "the zone state was made without a heat map"; return SS_ERR_INVALID; }
    if (!z->has_lut) { err = who + "no colour table (ss_zone_set_colormap)"; return SS_ERR_INVALID; }
    if (h != d.h || w != d.w) { err = who + "frame size differs from the zone state's"; return SS_ERR_INVALID; }
    if (heat_frame_stride != 0 && heat_frame_stride < (long long)d.gh * d.gw) { err = who + "heat_frame_stride must be 0 or at least the grid's cells"; return SS_ERR_INVALID; }
    if (batch == 0) return SS_OK;
    const long long rows = (long long)batch * h;
    hipLaunchKernelGGL(k_zone_heat_blend, dim3((unsigned)(rows < 2048 ? rows : 2048)), dim3(256), 0, st, d_frames, batch, frame_batch_stride, h, w, row_stride,
                       d_heat, heat_frame_stride, d_max, max_stride, d.k, d.gw, d.lut, (unsigned)alpha);
    SS_HIPCHK(who, hipGetLastError());
    return SS_OK;
}
