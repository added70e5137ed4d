// ss_jpeg.hip — baseline JPEG frames decoded into the pipeline's frame buffer (docs/JPEG.md).
//
// The host does the serial part only: headers, Huffman tables and the entropy-coded scan, whole images dealt out to the call's
// host threads.  What leaves the host is a SPARSE coefficient stream (a 32-bit offset per block, a 32-bit entry per non-zero
// coefficient), packed into a write-combined staging area and sent in one asynchronous copy.  Two kernels do the rest for all
// images of the call at once:
//   k_jpeg_idct    eight lanes per 8x8 block: expand the block's entries into LDS (dequantised), ISLOW pass 1 with lane = column,
//                  pass 2 with lane = row, range limit, 8 bytes per lane into the component planes
//   k_jpeg_pixels  a lane makes 4 consecutive pixels of the flat HWC image (12 bytes = 3 dwords): fancy chroma upsampling from
//                  the planes (neighbours across block borders included), YCbCr -> BGR / RGB, the store
// Every value is an integer; the results equal libjpeg-turbo's defaults (JDCT_ISLOW, fancy upsampling) bit for bit.
// On request the entropy-coded scan is decoded on the device as well (ss_jpeg_decode_batch_device: the second half of this file).
#include <cstring>
#include <string>
#include <vector>
#include "ss_common.h"
#include "ss_host.h"
#include "ss_launch.h"
#include "ss_jpeg_host.h"

#define JPEG_HDR 160                    // dwords of an image's header in the stream (see docs/JPEG.md "staging layout")
#define JPEG_WS_PITCH 72                // LDS dwords per block, rows of 9 (8 + 1 pad): the 32 lanes of a ds_read_b32 / ds_write_b32 group (4 blocks)
                                        // hit 32 different banks in pass 1 (lane = column) and in pass 2 (lane = row)

// ---- host: headers ---------------------------------------------------------------------------------------------------------
struct JHuff {
    bool present = false;
    uint16_t fast[512];                 // 9 leading bits -> (length << 8) | symbol, 0: the code is longer (or does not exist)
    int mincode[17], maxcode[17], valptr[17];
    uint8_t vals[256];
};

struct JInfo {
    int width = 0, height = 0, ncomp = 0;
    int cid[3], h[3], v[3], tq[3], td[3], ta[3];
    uint16_t quant[4][64];              // natural order
    bool have_q[4] = {false, false, false, false};
    JHuff dc[4], ac[4];
    int ri = 0;
    size_t scan = 0;                    // first byte of the entropy-coded data
    int mcux = 0, mcuy = 0;
};

static bool jfail(std::string& err, const std::string& msg) { err = msg; return false; }

static bool build_huff(JHuff& t, const uint8_t* counts, const uint8_t* syms, int tot)
{
    memset(t.fast, 0, sizeof t.fast);
    memcpy(t.vals, syms, tot);
    int code = 0, k = 0;
    for (int ln = 1; ln <= 16; ++ln) {
        t.valptr[ln] = k;
        t.mincode[ln] = code;
        if (counts[ln - 1] > (1 << ln) - code) return false;    // more codes of this length than the code space has left
        for (int i = 0; i < counts[ln - 1]; ++i, ++code, ++k)
            if (ln <= 9)
                for (int f = 0; f < (1 << (9 - ln)); ++f) t.fast[(code << (9 - ln)) | f] = (uint16_t)((ln << 8) | syms[k]);
        t.maxcode[ln] = counts[ln - 1] ? code - 1 : -1;
        code <<= 1;
    }
    t.present = true;
    return true;
}

static bool parse_headers(const uint8_t* d, size_t n, JInfo& J, std::string& err)
{
    if (n < 4 || d[0] != 0xFF || d[1] != 0xD8) return jfail(err, "no SOI marker");
    size_t p = 2;
    bool sof = false, jfif = false;
    int adobe = -1;
    const uint8_t* seg = nullptr;
    size_t L = 0;
    for (;;) {
        while (p < n && d[p] != 0xFF) ++p;
        while (p < n && d[p] == 0xFF) ++p;
        if (p >= n) return jfail(err, "no scan");
        const int m = d[p++];
        if (m == 0xD8 || m == 0x01 || (m >= 0xD0 && m <= 0xD7)) continue;
        if (m == 0xD9) return jfail(err, "no scan");
        if (p + 2 > n) return jfail(err, "truncated header");
        L = ((size_t)d[p] << 8) | d[p + 1];
        if (L < 2 || p + L > n) return jfail(err, "truncated header");
        seg = d + p + 2;
        const size_t sl = L - 2;
        if (m == 0xC0) {
            if (sof) return jfail(err, "two frame headers");
            if (sl < 6 || sl != 6 + 3 * (size_t)seg[5]) return jfail(err, "bad frame header");
            if (seg[0] != 8) return jfail(err, "12-bit samples");
            J.height = (seg[1] << 8) | seg[2];
            J.width = (seg[3] << 8) | seg[4];
            J.ncomp = seg[5];
            for (int i = 0; i < J.ncomp && i < 3; ++i) { J.cid[i] = seg[6 + 3 * i]; J.h[i] = seg[7 + 3 * i] >> 4; J.v[i] = seg[7 + 3 * i] & 15; J.tq[i] = seg[8 + 3 * i]; }
            sof = true;
        } else if (m >= 0xC1 && m <= 0xCF && m != 0xC4 && m != 0xC8 && m != 0xCC) {
            const char* kind = m == 0xC1 ? "extended sequential" : m == 0xC2 ? "progressive" : m == 0xC3 ? "lossless" : "arithmetic or differential";
            return jfail(err, std::string(kind) + " JPEG (SOF" + std::to_string(m - 0xC0) + ")");
        } else if (m == 0xCC) {
            return jfail(err, "arithmetic coding");
        } else if (m == 0xDB) {
            for (size_t q = 0; q < sl; q += 65) {
                const int pq = seg[q] >> 4, tq = seg[q] & 15;
                if (pq != 0) return jfail(err, "16-bit quantisation table");
                if (tq > 3 || q + 65 > sl) return jfail(err, "bad quantisation table");
                for (int k = 0; k < 64; ++k) J.quant[tq][kZigzag[k]] = seg[q + 1 + k];
                J.have_q[tq] = true;
            }
        } else if (m == 0xC4) {
            size_t q = 0;
            while (q < sl) {
                if (q + 17 > sl) return jfail(err, "bad Huffman table");
                const int tc = seg[q] >> 4, th = seg[q] & 15;
                int tot = 0;
                for (int i = 0; i < 16; ++i) tot += seg[q + 1 + i];
                if (tc > 1 || th > 3 || tot > 256 || q + 17 + tot > sl) return jfail(err, "bad Huffman table");
                if (!build_huff(tc ? J.ac[th] : J.dc[th], seg + q + 1, seg + q + 17, tot)) return jfail(err, "bad Huffman table");
                q += 17 + tot;
            }
        } else if (m == 0xDD) {
            if (sl != 2) return jfail(err, "bad restart interval");
            J.ri = (seg[0] << 8) | seg[1];
        } else if (m == 0xE0 && sl >= 5 && !memcmp(seg, "JFIF\0", 5)) {
            jfif = true;
        } else if (m == 0xEE && sl >= 12 && !memcmp(seg, "Adobe", 5)) {
            adobe = seg[11];
        } else if (m == 0xDA) {
            if (!sof) return jfail(err, "scan before the frame header");
            break;
        }
        p += L;
    }
    const size_t sl = L - 2;
    if (J.height < 1 || J.height > 8192 || J.width < 1 || J.width > 8192) return jfail(err, "sides must be 1 ... 8192");
    if (J.ncomp != 1 && J.ncomp != 3) return jfail(err, std::to_string(J.ncomp) + " components (1 or 3 are decoded)");
    if (adobe == 0 && J.ncomp == 3) return jfail(err, "Adobe marker with transform 0 (RGB)");
    if (J.ncomp == 3 && !jfif && adobe < 0 && J.cid[0] == 'R' && J.cid[1] == 'G' && J.cid[2] == 'B') return jfail(err, "component ids R, G, B (RGB)");
    if (J.ncomp == 1) {
        J.h[0] = J.v[0] = 1;                                   // a one-component scan is not interleaved: the factors do not matter
    } else {
        const bool luma = (J.h[0] == 1 && J.v[0] == 1) || (J.h[0] == 2 && J.v[0] == 1) || (J.h[0] == 2 && J.v[0] == 2);
        if (!luma || J.h[1] != 1 || J.v[1] != 1 || J.h[2] != 1 || J.v[2] != 1) {
            std::string s = "sampling factors";
            for (int i = 0; i < 3; ++i) s += " " + std::to_string(J.h[i]) + "x" + std::to_string(J.v[i]);
            return jfail(err, s + " (4:4:4, 4:2:2 and 4:2:0 are decoded)");
        }
    }
    if (sl < 1 || seg[0] != J.ncomp || sl != 4 + 2 * (size_t)seg[0]) return jfail(err, "several scans");
    if (seg[sl - 3] != 0 || seg[sl - 2] != 63 || seg[sl - 1] != 0) return jfail(err, "scan header is not a baseline one (Ss 0, Se 63, Ah / Al 0)");
    for (int i = 0; i < J.ncomp; ++i) {
        if (seg[1 + 2 * i] != J.cid[i]) return jfail(err, "scan components out of order");
        J.td[i] = seg[2 + 2 * i] >> 4;
        J.ta[i] = seg[2 + 2 * i] & 15;
    }
    for (int i = 0; i < J.ncomp; ++i) {
        if (J.tq[i] > 3 || !J.have_q[J.tq[i]]) return jfail(err, "missing quantisation table " + std::to_string(J.tq[i]));
        if (J.td[i] > 3 || !J.dc[J.td[i]].present) return jfail(err, "missing DC Huffman table " + std::to_string(J.td[i]));
        if (J.ta[i] > 3 || !J.ac[J.ta[i]].present) return jfail(err, "missing AC Huffman table " + std::to_string(J.ta[i]));
    }
    J.scan = p + L;
    J.mcux = (J.width + 8 * J.h[0] - 1) / (8 * J.h[0]);
    J.mcuy = (J.height + 8 * J.v[0] - 1) / (8 * J.v[0]);
    return true;
}

// ---- host: the entropy-coded scan ------------------------------------------------------------------------------------------
// Bits are held left-aligned in a 64-bit word.  At a marker (or the end of the data) the reader stops advancing and supplies zero
// bits, counted in `fake`: they are always the last bits of the word, so real data has run out exactly when cnt < fake.
struct JBits {
    const uint8_t* d;
    size_t pos, n;
    uint64_t buf = 0;
    int cnt = 0, fake = 0;
    bool marker = false;
    inline void fill()
    {
        if (cnt <= 32 && !marker && pos + 8 <= n) {              // eight bytes without an FF: whole bytes straight into the word
            uint64_t w;
            memcpy(&w, d + pos, 8);
            const uint64_t x = ~w;
            if (!((x - 0x0101010101010101ull) & ~x & 0x8080808080808080ull)) {
                const int k = (64 - cnt) >> 3;
                buf |= (__builtin_bswap64(w) >> cnt) & ~(((uint64_t)1 << (64 - cnt - 8 * k)) - 1);
                pos += k;
                cnt += 8 * k;
                return;
            }
        }
        while (cnt <= 56) {
            unsigned x = 0;
            if (!marker && pos < n) {
                x = d[pos];
                if (x != 0xFF) ++pos;
                else if (pos + 1 < n && d[pos + 1] == 0) pos += 2;
                else { marker = true; x = 0; }
            } else marker = true;
            if (marker) fake += 8;
            buf |= (uint64_t)x << (56 - cnt);
            cnt += 8;
        }
    }
    inline unsigned peek(int k) const { return (unsigned)(buf >> (64 - k)); }
    inline void skip(int k) { buf <<= k; cnt -= k; }
};

static inline int huff_sym(JBits& b, const JHuff& t)            // after fill(); -1: no such code
{
    const unsigned f = t.fast[b.peek(9)];
    if (f) { b.skip(f >> 8); return f & 255; }
    for (int ln = 10; ln <= 16; ++ln) {
        const int code = (int)b.peek(ln);
        if (t.maxcode[ln] >= 0 && code <= t.maxcode[ln] && code >= t.mincode[ln]) { b.skip(ln); return t.vals[t.valptr[ln] + code - t.mincode[ln]]; }
    }
    return -1;
}

static inline int receive_extend(JBits& b, int s)               // 1 <= s <= 15
{
    const int v = (int)b.peek(s);
    b.skip(s);
    return v >= (1 << (s - 1)) ? v : v - (1 << s) + 1;
}

// Sink: begin(ci, by, bx) opens the next block in scan order, coef(k_natural, value) adds one of its non-zero coefficients.
template <class Sink>
static bool decode_scan(const uint8_t* d, size_t n, const JInfo& J, Sink& sink, std::string& err)
{
    JBits b{d, J.scan, n};
    int pred[3] = {0, 0, 0};
    const int nm = J.mcux * J.mcuy;
    int rst = 0;
    for (int m = 0; m < nm; ++m) {
        if (J.ri && m && m % J.ri == 0) {
            b.fill();
            if (b.cnt - b.fake >= 8 || !b.marker) return jfail(err, "bad restart marker");
            size_t q = b.pos;
            while (q < n && d[q] == 0xFF) ++q;
            if (q >= n || q == b.pos || d[q] != 0xD0 + (rst & 7)) return jfail(err, "bad restart marker");
            ++rst;
            b = JBits{d, q + 1, n};
            pred[0] = pred[1] = pred[2] = 0;
        }
        const int my = m / J.mcux, mx = m % J.mcux;
        for (int ci = 0; ci < J.ncomp; ++ci) {
            const JHuff &dc = J.dc[J.td[ci]], &ac = J.ac[J.ta[ci]];
            for (int by = 0; by < J.v[ci]; ++by)
                for (int bx = 0; bx < J.h[ci]; ++bx) {
                    sink.begin(ci, my * J.v[ci] + by, mx * J.h[ci] + bx);
                    b.fill();
                    int c0 = b.cnt;                               // c0 <= b.fake: the symbol starts beyond the last real bit; it is not judged, the data has ended
                    int s = huff_sym(b, dc);
                    if (s < 0) return jfail(err, b.cnt - b.fake < 16 ? "data ends before the last MCU" : "Huffman code that does not exist");
                    if (s > 15) return jfail(err, c0 <= b.fake ? "data ends before the last MCU" : "bad DC category");
                    if (s) pred[ci] += receive_extend(b, s);
                    pred[ci] = (int16_t)pred[ci];
                    if (pred[ci]) sink.coef(0, pred[ci]);
                    for (int k = 1; k < 64;) {
                        b.fill();
                        c0 = b.cnt;
                        const int rs = huff_sym(b, ac);
                        if (rs < 0) return jfail(err, b.cnt - b.fake < 16 ? "data ends before the last MCU" : "Huffman code that does not exist");
                        const int r = rs >> 4;
                        s = rs & 15;
                        if (!s) {
                            if (r != 15) break;
                            k += 16;
                            continue;
                        }
                        k += r;
                        if (k > 63) return jfail(err, c0 <= b.fake ? "data ends before the last MCU" : "coefficient index beyond 63");
                        const int v = receive_extend(b, s);
                        if (v) sink.coef(kZigzag[k], v);
                        ++k;
                    }
                    if (b.cnt < b.fake) return jfail(err, "data ends before the last MCU");
                }
        }
    }
    return true;
}

int ss_jpeg_probe_impl(const unsigned char* data, size_t size, int* width, int* height, int* components, int* h_samp, int* v_samp, std::string& err)
{
    JInfo* J = new (std::nothrow) JInfo();
    if (!J) { err = "out of memory"; return SS_ERR_INVALID; }
    const bool ok = parse_headers(data, size, *J, err);
    if (ok) { *width = J->width; *height = J->height; *components = J->ncomp; *h_samp = J->h[0]; *v_samp = J->v[0]; }
    delete J;
    return ok ? SS_OK : SS_ERR_INVALID;
}

struct DenseSink {
    short* coef_out;
    size_t base[3];
    int bw[3];
    short* cur = nullptr;
    void begin(int ci, int by, int bx) { cur = coef_out + base[ci] + ((size_t)by * bw[ci] + bx) * 64; }
    void coef(int k, int v) { cur[k] = (short)v; }
};

int ss_jpeg_coefficients_impl(const unsigned char* data, size_t size, short* coef, size_t coef_cap, unsigned short* quant, std::string& err)
{
    JInfo* J = new (std::nothrow) JInfo();
    if (!J) { err = "out of memory"; return SS_ERR_INVALID; }
    int rc = SS_ERR_INVALID;
    if (parse_headers(data, size, *J, err)) {
        DenseSink sink{coef, {0, 0, 0}, {0, 0, 0}};
        size_t tot = 0;
        for (int c = 0; c < J->ncomp; ++c) { sink.base[c] = tot; sink.bw[c] = J->mcux * J->h[c]; tot += (size_t)J->mcux * J->h[c] * J->mcuy * J->v[c] * 64; }
        if (tot > coef_cap) err = "coefficient buffer too small: " + std::to_string(tot) + " values needed";
        else {
            memset(coef, 0, tot * sizeof(short));
            memset(quant, 0, 4 * 64 * sizeof(unsigned short));
            for (int t = 0; t < 4; ++t) if (J->have_q[t]) memcpy(quant + 64 * t, J->quant[t], 64 * sizeof(unsigned short));
            if (decode_scan(data, size, *J, sink, err)) rc = SS_OK;
        }
    }
    delete J;
    return rc;
}

// ---- device ----------------------------------------------------------------------------------------------------------------
// The stream (dwords; every image's header first, then per image its block table and its entries):
//   header i at JPEG_HDR * i:  [0] components  [1] h  [2] v (luma factors)  [3] MCUs per row  [4] blocks  [5] block table (dword index)
//                              [6] entries (dword index)  [8 + c] quantisation table of component c  [11 + c] plane offset (bytes)
//                              [14 + c] plane pitch  [32 .. 160) the four quantisation tables, uint16 [4][64], natural order
//   block table:  blocks + 1 dwords in SCAN order; block b's entries are entries[table[b] .. table[b + 1])
//   entry:        (natural-order index << 16) | (uint16) value
__device__ __forceinline__ void jpeg_pass(uint32_t (&x)[8], int s)
{
    const uint32_t a = 2446, b = 3196, c = 4433, dd = 6270, e = 7373, f = 9633, g = 12299, h = 15137, i = 16069, j = 16819, k = 20995, l = 25172;
    const uint32_t r = 1u << (s - 1);
    uint32_t z1 = (x[2] + x[6]) * c;
    const uint32_t t2 = z1 - x[6] * h, t3 = z1 + x[2] * dd, t0 = (x[0] + x[4]) << 13, t1 = (x[0] - x[4]) << 13;
    const uint32_t t10 = t0 + t3, t13 = t0 - t3, t11 = t1 + t2, t12 = t1 - t2;
    uint32_t o0 = x[7], o1 = x[5], o2 = x[3], o3 = x[1];
    z1 = o0 + o3;
    uint32_t z2 = o1 + o2, z3 = o0 + o2, z4 = o1 + o3;
    const uint32_t z5 = (z3 + z4) * f;
    o0 *= a; o1 *= j; o2 *= l; o3 *= g;
    z1 = 0u - z1 * e; z2 = 0u - z2 * k; z3 = z5 - z3 * i; z4 = z5 - z4 * b;
    o0 += z1 + z3; o1 += z2 + z4; o2 += z2 + z3; o3 += z1 + z4;
    x[0] = (uint32_t)((int32_t)(t10 + o3 + r) >> s); x[7] = (uint32_t)((int32_t)(t10 - o3 + r) >> s);
    x[1] = (uint32_t)((int32_t)(t11 + o2 + r) >> s); x[6] = (uint32_t)((int32_t)(t11 - o2 + r) >> s);
    x[2] = (uint32_t)((int32_t)(t12 + o1 + r) >> s); x[5] = (uint32_t)((int32_t)(t12 - o1 + r) >> s);
    x[3] = (uint32_t)((int32_t)(t13 + o0 + r) >> s); x[4] = (uint32_t)((int32_t)(t13 - o0 + r) >> s);
}

__device__ __forceinline__ uint32_t jpeg_limit(uint32_t y)
{
    const uint32_t v = y & 1023u;
    return v < 128u ? v + 128u : v < 512u ? 255u : v < 896u ? 0u : v - 896u;
}

// grid (ceil(max blocks / 32), images), 256 threads: 8 lanes per block, 32 blocks per workgroup
__global__ __launch_bounds__(256) void k_jpeg_idct(const uint32_t* __restrict__ s, uint8_t* __restrict__ planes, long long plane_slot)
{
    __shared__ uint32_t ws[32 * JPEG_WS_PITCH];
    const uint32_t* hdr = s + (size_t)blockIdx.y * JPEG_HDR;
    const int nblk = (int)hdr[4], lb = threadIdx.x >> 3, l = threadIdx.x & 7, blk = blockIdx.x * 32 + lb;
    const bool on = blk < nblk;
    uint32_t* w = ws + lb * JPEG_WS_PITCH;
    // the block's place: scan order -> (component, block row, block column)
    const int h = (int)hdr[1], v = (int)hdr[2], mcux = (int)hdr[3], ncomp = (int)hdr[0];
    const int bpm = ncomp == 1 ? 1 : h * v + 2, mcu = blk / bpm, jj = blk - mcu * bpm, my = mcu / mcux, mx = mcu - my * mcux;
    int comp = 0, by = my, bx = mx;
    if (jj < h * v) { by = my * v + jj / h; bx = mx * h + jj % h; }
    else comp = 1 + jj - h * v;
#pragma unroll
    for (int i = 0; i < 8; ++i) w[l * 9 + i] = 0u;
    __syncthreads();
    if (on) {
        const uint32_t* tab = s + hdr[5];
        const uint32_t* ent = s + hdr[6];
        const uint16_t* q = (const uint16_t*)(hdr + 32) + 64 * hdr[8 + comp];
        const uint32_t e1 = tab[blk + 1];
        for (uint32_t e = tab[blk] + l; e < e1; e += 8) {
            const uint32_t u = ent[e], k = (u >> 16) & 63u;
            w[(k >> 3) * 9 + (k & 7)] = (uint32_t)(int32_t)(int16_t)(u & 0xffffu) * (uint32_t)q[k];
        }
    }
    __syncthreads();
    uint32_t x[8];
#pragma unroll
    for (int i = 0; i < 8; ++i) x[i] = w[i * 9 + l];             // lane = column
    jpeg_pass(x, 11);
#pragma unroll
    for (int i = 0; i < 8; ++i) w[i * 9 + l] = x[i];
    __syncthreads();
#pragma unroll
    for (int i = 0; i < 8; ++i) x[i] = w[l * 9 + i];             // lane = row
    jpeg_pass(x, 18);
    if (on) {
        uint2 o;
        o.x = jpeg_limit(x[0]) | jpeg_limit(x[1]) << 8 | jpeg_limit(x[2]) << 16 | jpeg_limit(x[3]) << 24;
        o.y = jpeg_limit(x[4]) | jpeg_limit(x[5]) << 8 | jpeg_limit(x[6]) << 16 | jpeg_limit(x[7]) << 24;
        uint8_t* p = planes + (size_t)blockIdx.y * plane_slot + hdr[11 + comp] + (size_t)(by * 8 + l) * hdr[14 + comp] + (size_t)bx * 8;
        *(uint2*)p = o;                                          // plane offsets and pitches are multiples of 8
    }
}

// One chroma sample of the full-size image at (x, y): libjpeg's fancy (triangle) upsampling, replication for planes at most 2 wide
__device__ __forceinline__ int jpeg_chroma(const uint8_t* __restrict__ p, int pitch, int cw, int ch, int x, int y, int hs, int vs)
{
    if (hs == 1) return p[y * pitch + x];
    const int cx = x >> 1, cy = vs == 2 ? y >> 1 : y;
    if (cw <= 2) return p[cy * pitch + cx];
    const int xn = (x & 1) ? min(cx + 1, cw - 1) : max(cx - 1, 0);
    if (vs == 1) return (3 * p[cy * pitch + cx] + p[cy * pitch + xn] + ((x & 1) ? 2 : 1)) >> 2;
    const int oy = (y & 1) ? min(cy + 1, ch - 1) : max(cy - 1, 0);
    const int c0 = 3 * p[cy * pitch + cx] + p[oy * pitch + cx], c1 = 3 * p[cy * pitch + xn] + p[oy * pitch + xn];
    return (3 * c0 + c1 + ((x & 1) ? 7 : 8)) >> 4;
}

__device__ __forceinline__ uint32_t jpeg_clamp(int v) { return (uint32_t)min(max(v, 0), 255); }

// grid (ceil(ceil(H W / 4) / 256), images), 256 threads: a lane makes pixels 4 g .. 4 g + 3 of the flat image (rows are contiguous
// in HWC, so the 12 bytes are three aligned dwords whenever the image's base is; otherwise, and at the ragged end, bytes)
__global__ __launch_bounds__(256) void k_jpeg_pixels(const uint32_t* __restrict__ s, const uint8_t* __restrict__ planes, long long plane_slot,
                                                     int H, int W, uint8_t* __restrict__ out, long long out_stride, int rgb, int dwords)
{
    const uint32_t* hdr = s + (size_t)blockIdx.y * JPEG_HDR;
    const int g = blockIdx.x * 256 + threadIdx.x, npix = H * W, p0 = 4 * g;
    if (p0 >= npix) return;
    const int ncomp = (int)hdr[0], hs = (int)hdr[1], vs = (int)hdr[2];
    const uint8_t* base = planes + (size_t)blockIdx.y * plane_slot;
    const uint8_t *py = base + hdr[11], *pb = base + hdr[12], *pr = base + hdr[13];
    const int ypitch = (int)hdr[14], cpitch = (int)hdr[15], cw = (W + hs - 1) / hs, ch = (H + vs - 1) / vs;
    uint32_t px[4];
    int y = p0 / W, x = p0 - y * W;
#pragma unroll
    for (int i = 0; i < 4; ++i) {
        px[i] = 0;
        if (p0 + i < npix) {
            const int Y = py[y * ypitch + x];
            if (ncomp == 1) px[i] = (uint32_t)Y * 0x010101u;
            else {
                const int cb = jpeg_chroma(pb, cpitch, cw, ch, x, y, hs, vs) - 128, cr = jpeg_chroma(pr, cpitch, cw, ch, x, y, hs, vs) - 128;
                const uint32_t R = jpeg_clamp(Y + ((91881 * cr + 32768) >> 16)), G = jpeg_clamp(Y + ((-22554 * cb - 46802 * cr + 32768) >> 16)),
                               B = jpeg_clamp(Y + ((116130 * cb + 32768) >> 16));
                px[i] = rgb ? (R | G << 8 | B << 16) : (B | G << 8 | R << 16);
            }
        }
        if (++x == W) { x = 0; ++y; }
    }
    uint8_t* o = out + (size_t)blockIdx.y * out_stride + (size_t)p0 * 3;
    if (dwords && p0 + 4 <= npix) {
        uint32_t* o4 = (uint32_t*)o;
        o4[0] = px[0] | px[1] << 24;
        o4[1] = px[1] >> 8 | px[2] << 16;
        o4[2] = px[2] >> 16 | px[3] << 8;
    } else {
        for (int i = 0; i < 4 && p0 + i < npix; ++i) { o[3 * i] = (uint8_t)px[i]; o[3 * i + 1] = (uint8_t)(px[i] >> 8); o[3 * i + 2] = (uint8_t)(px[i] >> 16); }
    }
}

// ---- host: the batch call --------------------------------------------------------------------------------------------------
struct SparseSink {
    std::vector<uint32_t>*tab, *ent;
    void begin(int, int, int) { tab->push_back((uint32_t)ent->size()); }
    void coef(int k, int v) { ent->push_back((uint32_t)k << 16 | (uint32_t)(uint16_t)(int16_t)v); }
};

struct SSJpeg {
    struct Slot {
        SsBuf<SS_PINNED_WC> host;                               // staging
        SsBuf<SS_DEVICE> dev;                                   // its device mirror
        SsBuf<SS_DEVICE> planes;                                // component planes of the call's images
        SsEvent ev; bool busy = false;
        SsBuf<SS_DEVICE> status_dev;                            // device entropy stage: a status word per image
        SsBuf<SS_PINNED> status_host;                           // and its pinned copy
        int pending = 0;                                        // images whose status arrives with `ev` (0: the call was a host-stage one)
    } slot[2];
    int next = 0;
    std::vector<int> rounds;                                    // ss_jpeg_device_coefficients: rounds each tile of its image took
    struct Image { JInfo J; std::vector<uint32_t> tab, ent; std::string err; bool ok = false; size_t tab_at = 0, ent_at = 0; };
    std::vector<Image> img;
};

void ss_jpeg_free(SSJpeg* j) { delete j; }

static const char* const kJpegWho = "ss_jpeg_decode_batch: ";      // HIP failures of both batch paths are reported under this name

static int jpeg_slot_wait(SSJpeg::Slot& st, std::string& err);

// what both batch paths keep in a slot: the staging area and its mirror with a quarter to spare, the planes exact
static int jpeg_slot_reserve(SSJpeg::Slot& st, size_t host_bytes, size_t dev_bytes, size_t planes_bytes, std::string& err)
{
    SS_HIPCHK(kJpegWho, st.host.reserve(host_bytes, SS_QUARTER));
    SS_HIPCHK(kJpegWho, st.dev.reserve(dev_bytes, SS_QUARTER));
    SS_HIPCHK(kJpegWho, st.planes.reserve(planes_bytes, SS_EXACT));
    return SS_OK;
}

// The arguments have been checked (ss_api.hip).  Returns an SS_* code, the message in err.
int ss_jpeg_decode_impl(SSJpeg** state, hipStream_t stream, const unsigned char* const* data, const size_t* sizes, int n, int height, int width,
                        void* d_out, long long out_frame_stride, int rgb, int threads, std::string& err)
{
    try {
        if (!*state) *state = new SSJpeg();
        SSJpeg& S = **state;
        if ((int)S.img.size() < n) S.img.resize(n);
        // ---- 1. headers + entropy decoding, whole images per thread ----
        auto decode = [&S, data, sizes, n, height, width](int t, int nt) {
            for (int i = t; i < n; i += nt) {
                SSJpeg::Image& im = S.img[i];
                im.ok = false;
                im.err.clear();
                im.tab.clear();
                im.ent.clear();
                try {
                    im.J = JInfo();
                    if (!parse_headers(data[i], sizes[i], im.J, im.err)) continue;
                    if (im.J.width != width || im.J.height != height) {
                        im.err = "size " + std::to_string(im.J.width) + "x" + std::to_string(im.J.height) + " differs from the batch's " + std::to_string(width) + "x" + std::to_string(height);
                        continue;
                    }
                    SparseSink sink{&im.tab, &im.ent};
                    if (!decode_scan(data[i], sizes[i], im.J, sink, im.err)) continue;
                    im.tab.push_back((uint32_t)im.ent.size());
                    im.ok = true;
                } catch (...) {
                    im.err = "out of memory";
                }
            }
        };
        const int T = threads < n ? threads : n;
        if (!run_threads(T, decode)) { err = "ss_jpeg_decode_batch: host decoding failed"; return SS_ERR_INVALID; }
        for (int i = 0; i < n; ++i)
            if (!S.img[i].ok) { err = "ss_jpeg_decode_batch: image " + std::to_string(i) + ": " + S.img[i].err; return SS_ERR_INVALID; }
        // ---- 2. layout ----
        size_t at = (size_t)n * JPEG_HDR;
        int max_blk = 0;
        for (int i = 0; i < n; ++i) {
            SSJpeg::Image& im = S.img[i];
            im.tab_at = at; at += im.tab.size();
            im.ent_at = at; at += im.ent.size();
            if ((int)im.tab.size() - 1 > max_blk) max_blk = (int)im.tab.size() - 1;
        }
        if (at >= ((size_t)1 << 32)) { err = "ss_jpeg_decode_batch: coefficient stream beyond 2^32 entries"; return SS_ERR_CAPACITY; }
        const size_t bytes = at * 4;
        const size_t plane_slot = 3 * (size_t)((width + 15) / 16 * 16) * ((height + 15) / 16 * 16), planes_bytes = plane_slot * n;
        SSJpeg::Slot& st = S.slot[S.next];
        if (int rcw = jpeg_slot_wait(st, err)) return rcw;       // (a device-entropy call that used this slot may have refused an image)
        SS_HIPCHK(kJpegWho, st.ev.ensure());
        if (int rcr = jpeg_slot_reserve(st, bytes, bytes, planes_bytes, err)) return rcr;
        // ---- 3. pack into the write-combined area (sequential stores only) ----
        uint32_t* base = st.host.as<uint32_t>();
        auto pack = [&S, base, n](int t, int nt) {
            for (int i = t; i < n; i += nt) {
                const SSJpeg::Image& im = S.img[i];
                const JInfo& J = im.J;
                uint32_t hdr[JPEG_HDR];
                memset(hdr, 0, sizeof hdr);
                hdr[0] = J.ncomp; hdr[1] = J.h[0]; hdr[2] = J.v[0]; hdr[3] = J.mcux; hdr[4] = (uint32_t)im.tab.size() - 1;
                hdr[5] = (uint32_t)im.tab_at; hdr[6] = (uint32_t)im.ent_at;
                uint32_t off = 0;
                for (int c = 0; c < J.ncomp; ++c) {
                    const uint32_t pitch = J.mcux * J.h[c] * 8, rows = J.mcuy * J.v[c] * 8;
                    hdr[8 + c] = J.tq[c]; hdr[11 + c] = off; hdr[14 + c] = pitch;
                    off += pitch * rows;
                }
                memcpy(hdr + 32, J.quant, sizeof J.quant);
                memcpy(base + (size_t)i * JPEG_HDR, hdr, sizeof hdr);
                memcpy(base + im.tab_at, im.tab.data(), im.tab.size() * 4);
                if (!im.ent.empty()) memcpy(base + im.ent_at, im.ent.data(), im.ent.size() * 4);
            }
        };
        if (!run_threads(bytes < ((size_t)1 << 20) ? 1 : T, pack)) { err = "ss_jpeg_decode_batch: host staging failed"; return SS_ERR_INVALID; }
        // ---- 4. one copy, two launches ----
        uint32_t* dev = st.dev.as<uint32_t>();
        uint8_t* planes = st.planes.as<uint8_t>();
        SS_HIPCHK(kJpegWho, hipMemcpyAsync(dev, base, bytes, hipMemcpyHostToDevice, stream));
        hipLaunchKernelGGL(k_jpeg_idct, dim3((max_blk + 31) / 32, n), dim3(256), 0, stream, dev, planes, (long long)plane_slot);
        const int groups = (height * width + 3) / 4;
        const int dwords = (((uintptr_t)d_out | (uintptr_t)out_frame_stride) & 3) == 0;
        hipLaunchKernelGGL(k_jpeg_pixels, dim3((groups + 255) / 256, n), dim3(256), 0, stream, dev, planes, (long long)plane_slot, height, width,
                           (uint8_t*)d_out, out_frame_stride, rgb, dwords);
        SS_HIPCHK(kJpegWho, hipGetLastError());
        SS_HIPCHK(kJpegWho, hipEventRecord(st.ev, stream));
        st.busy = true;
        S.next ^= 1;
        return SS_OK;
    } catch (...) {
        err = "ss_jpeg_decode_batch: out of memory";
        return SS_ERR_INVALID;
    }
}

// ============================================================================================================================
// The entropy stage on the device (docs/JPEG.md section 12; tests/jpeg_huff_ref.py is the same algorithm in NumPy).
//
// The host keeps what is serial and cheap per file: the headers, the Huffman look-up tables and ONE pass over the scan that drops
// the stuffing bytes and cuts the scan at its restart markers into segments.  The entropy-coded bytes cross PCIe; two kernels make
// section 3's stream (block table + entries) in device memory, k_jpeg_idct and k_jpeg_pixels read it unchanged.
//   k_jpeg_huff   a workgroup per image, 1024 lanes, a lane per subsequence of W dwords of a segment: speculative decoding until
//                 every lane's entry state equals its left neighbour's exit state, a scan of the block and entry counts, then the
//                 pass that stores the block table and the entries (the DC slot of a block holds the raw DC difference)
//   k_jpeg_dc     per image and component the running sum of the DC differences, restarted at every segment; a refused image
//                 gets a block table of zeros instead (every block empty)
// Header words of the device stage (beside section 3's, which end at [16], the third component's pitch):  [17] segments  [18] scan
// bytes (dword index)  [19] Huffman tables (dword index; component c: DC at 2 c, AC at 2 c + 1)  [20] lanes  [21] entry capacity
// [22] rounds read-out (dword index, one per tile)  [23] W  [24] MCUs per segment  [25] segment table (dword index)
#define JH_TAB 344                      // dwords of a Huffman table: fast[512] uint16 | maxcode, mincode, valptr of the lengths 10 .. 16 (8 dwords each) | vals[256] uint8
#define JH_SEG 5                        // dwords of a segment: byte offset in the image's scan bytes, byte length, first block, blocks, first lane
#define JH_LANES 1024
#define JH_OK 0xffffffffu
enum { JE_CODE = 1, JE_DCCAT = 2, JE_INDEX = 3, JE_ENDS = 4, JE_RST = 5, JE_CAP = 6 };
static const char* const kJpegCause[7] = {"", "Huffman code that does not exist", "bad DC category", "coefficient index beyond 63", "data ends before the last MCU",
                                          "bad restart marker", "more entries than the scan's length allows"};

int g_opt_jpeg_subseq_words = 32;       // ss_op_set_option "jpeg_subseq_words": 4, 8, 16 or 32 dwords of scan per lane

__constant__ uint8_t d_jpeg_zigzag[64] = {0, 1, 8, 16, 9, 2, 3, 10, 17, 24, 32, 25, 18, 11, 4, 5, 12, 19, 26, 33, 40, 48, 41, 34, 27, 20, 13, 6, 7, 14, 21, 28,
                                          35, 42, 49, 56, 57, 50, 43, 36, 29, 22, 15, 23, 30, 37, 44, 51, 58, 59, 52, 45, 38, 31, 39, 46, 53, 60, 61, 54, 47, 55, 62, 63};

struct JhLane {                          // what a lane knows about its subsequence
    const uint32_t* w;                  // the segment's bytes (dwords, bytes in stream order)
    uint32_t nw;                        // dwords of the segment (padded length / 4): reads beyond supply zero bits
    uint32_t bits;                      // 8 * byte length: real data ends here
    uint32_t end;                       // symbols that start before this bit are the lane's
    int hv, bpm;                        // luma blocks per MCU, blocks per MCU
};

struct JhSink {                          // the storing pass
    uint32_t *tab, *ent;
    uint32_t e, cap;                    // next entry, capacity
    uint32_t blk, bend;                 // next block to begin (image-wide scan index), the segment's end
    bool last_seg;
    uint32_t err;
};

// Decodes from (p, bi, k) every symbol that starts before L.end, beginning at most `maxbegin` blocks.  Total: a code that does not
// exist consumes one bit, a DC category above 15 keeps its low four bits, a run beyond index 63 closes the block.
template <bool WRITE>
__device__ __forceinline__ void jh_decode(const uint32_t* tabs, const JhLane& L, uint32_t& p, uint32_t& bi, uint32_t& k, int maxbegin, uint32_t& nb, uint32_t& ne,
                                          uint32_t& nel, JhSink& S)
{
    nb = 0; ne = 0; nel = 0;
    uint32_t ci = 0xffffffffu, ca = 0, cb = 0;
    while (p < L.end) {
        if (k == 0 && (int)nb >= maxbegin) break;
        const uint32_t i = p >> 5, sh = p & 31u;
        if (i != ci) {
            ci = i;
            ca = i < L.nw ? __builtin_bswap32(L.w[i]) : 0u;
            cb = i + 1 < L.nw ? __builtin_bswap32(L.w[i + 1]) : 0u;
        }
        const uint32_t win = sh ? (ca << sh) | (cb >> (32u - sh)) : ca;
        const uint32_t comp = (int)bi < L.hv ? 0u : bi - (uint32_t)L.hv + 1u;
        const uint32_t* T = tabs + (2u * comp + (k ? 1u : 0u)) * JH_TAB;
        const uint32_t f = ((const uint16_t*)T)[win >> 23];
        uint32_t len = f >> 8, sym = f & 255u;
        if (!f) {
#pragma unroll
            for (int ln = 10; ln <= 16; ++ln) {
                const uint32_t code = win >> (32 - ln), mn = T[264 + ln - 10];
                if (!len && (int)code <= (int)T[256 + ln - 10] && code >= mn) { len = ln; sym = ((const uint8_t*)(T + 280))[(T[272 + ln - 10] + code - mn) & 255u]; }
            }
            if (!len) {
                if (WRITE && !S.err) S.err = L.bits - p < 16u ? JE_ENDS : JE_CODE;
                ++p;
                continue;
            }
        }
        bool close = false;
        if (k == 0) {
            uint32_t s = sym;
            if (s > 15u) { if (WRITE && !S.err) S.err = JE_DCCAT; s &= 15u; }
            uint32_t v = 0;
            if (s) { v = (win << len) >> (32u - s); if (v < (1u << (s - 1u))) v = v - (1u << s) + 1u; }
            nel = ne;
            if (WRITE) {
                if (S.e < S.cap) { S.tab[S.blk] = S.e; S.ent[S.e] = v & 0xffffu; }
                else if (!S.err) S.err = JE_CAP;
                ++S.blk; ++S.e;
            }
            ++nb; ++ne;
            p += len + s;
            k = 1;
        } else {
            const uint32_t r = sym >> 4, s = sym & 15u;
            if (!s) {
                p += len;
                if (r == 15u) { k += 16u; close = k > 63u; }
                else close = true;
            } else {
                k += r;
                if (k > 63u) {
                    if (WRITE && !S.err) S.err = JE_INDEX;
                    p += len;
                    close = true;
                } else {
                    uint32_t v = (win << len) >> (32u - s);
                    if (v < (1u << (s - 1u))) v = v - (1u << s) + 1u;
                    if (WRITE) {
                        if (S.e < S.cap) S.ent[S.e] = (uint32_t)d_jpeg_zigzag[k] << 16 | (v & 0xffffu);
                        else if (!S.err) S.err = JE_CAP;
                        ++S.e;
                    }
                    ++ne;
                    p += len + s;
                    close = ++k == 64u;
                }
            }
        }
        if (close) {
            k = 0;
            bi = (int)bi + 1 == L.bpm ? 0u : bi + 1u;
            if (WRITE && S.blk == S.bend) {                      // the segment's last block: what is left over?
                if (p > L.bits) { if (!S.err) S.err = JE_ENDS; }
                else if (!S.last_seg && L.bits - p >= 8u) { if (!S.err) S.err = JE_RST; }
                break;
            }
        }
    }
}

// inclusive sum over the workgroup's 1024 lanes (two barriers)
__device__ __forceinline__ uint32_t jh_scan(uint32_t v, uint32_t* wsum, uint32_t& total)
{
    const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
#pragma unroll
    for (int d = 1; d < 64; d <<= 1) {
        const uint32_t t = __shfl_up(v, d, 64);
        if (lane >= d) v += t;
    }
    if (lane == 63) wsum[wv] = v;
    __syncthreads();
    uint32_t off = 0, tot = 0;
#pragma unroll
    for (int i = 0; i < 16; ++i) { const uint32_t t = wsum[i]; if (i < wv) off += t; tot += t; }
    __syncthreads();
    total = tot;
    return v + off;
}

// grid (images), 1024 threads
__global__ __launch_bounds__(JH_LANES) void k_jpeg_huff(uint32_t* __restrict__ s, uint32_t* __restrict__ status)
{
    __shared__ uint32_t tabs[6 * JH_TAB];
    __shared__ uint32_t xp[JH_LANES], xs[JH_LANES], sc[JH_LANES];
    __shared__ uint32_t wsum[16], bc[1];
    const uint32_t* hdr = s + (size_t)blockIdx.x * JPEG_HDR;
    const int tid = threadIdx.x, ncomp = (int)hdr[0];
    const uint32_t blocks = hdr[4], nseg = hdr[17], lanes = hdr[20], W = hdr[23];
    const uint32_t* segs = s + hdr[25];
    const uint32_t* scan = s + hdr[18];
    uint32_t* rounds_out = s + hdr[22];
    for (int i = tid; i < ncomp * 2 * JH_TAB; i += JH_LANES) tabs[i] = s[hdr[19] + i];
    JhLane L;
    L.hv = ncomp == 1 ? 1 : (int)(hdr[1] * hdr[2]);
    L.bpm = ncomp == 1 ? 1 : L.hv + 2;
    JhSink S;
    S.tab = s + hdr[5]; S.ent = s + hdr[6]; S.cap = hdr[21];
    uint32_t cp = 0, cbk = 0, cblk = 0, cent = 0;               // carried from tile to tile: exit state, blocks begun in the open segment, entries
    __syncthreads();
    for (uint32_t tile0 = 0, t = 0; tile0 < lanes; tile0 += JH_LANES, ++t) {
        const uint32_t g = tile0 + tid, nl = lanes - tile0 < JH_LANES ? lanes - tile0 : JH_LANES;
        const bool active = g < lanes;
        uint32_t lane0 = 0, seg_blk0 = 0, seg_nblk = 0, j = 0;
        bool lastlane = false;
        L.w = scan; L.nw = 0; L.bits = 0; L.end = 0;
        if (active) {
            uint32_t lo = 0, hi = nseg - 1;
            for (int it = 0; it < 32 && lo < hi; ++it) {         // the last segment whose first lane is <= g
                const uint32_t mid = (lo + hi + 1) >> 1;
                if (segs[mid * JH_SEG + 4] <= g) lo = mid; else hi = mid - 1;
            }
            const uint32_t* sg = segs + lo * JH_SEG;
            const uint32_t len = sg[1];
            lane0 = sg[4]; seg_blk0 = sg[2]; seg_nblk = sg[3];
            j = g - lane0;
            L.w = scan + (sg[0] >> 2);
            L.nw = (len + 3) >> 2;
            L.bits = len << 3;
            const uint32_t e1 = (j + 1) * 32u * W;
            L.end = e1 < L.bits ? e1 : L.bits;
            lastlane = (lo + 1 == nseg ? lanes : sg[JH_SEG + 4]) == g + 1;
            S.last_seg = lo + 1 == nseg;
        }
        // ---- speculation: round 0 from the guess, then from the left neighbour's exit state while it differs ----
        const bool exact = j == 0 || tid == 0;
        uint32_t ep = j * 32u * W, ebk = 0;
        if (j != 0 && tid == 0) { ep = cp; ebk = cbk; }
        uint32_t p = ep, bi = ebk >> 8, k = ebk & 255u, nb = 0, ne = 0, nel = 0;
        if (active) jh_decode<false>(tabs, L, p, bi, k, 0x7fffffff, nb, ne, nel, S);
        xp[tid] = p; xs[tid] = bi << 8 | k;
        __syncthreads();
        uint32_t rounds = 1;
        for (uint32_t r = 1; r < nl; ++r) {                      // counted: lane i is final after i rounds
            uint32_t np = 0, nbk = 0;
            bool redo = false;
            if (active && !exact) { np = xp[tid - 1]; nbk = xs[tid - 1]; redo = np != ep || nbk != ebk; }
            if (!__syncthreads_or(redo)) break;
            ++rounds;
            if (redo) {
                ep = np; ebk = nbk;
                p = ep; bi = ebk >> 8; k = ebk & 255u;
                jh_decode<false>(tabs, L, p, bi, k, 0x7fffffff, nb, ne, nel, S);
                xp[tid] = p; xs[tid] = bi << 8 | k;
            }
            __syncthreads();
        }
        if (tid == 0) rounds_out[t] = rounds;
        // ---- where the lane's blocks and entries go ----
        uint32_t total;
        const uint32_t bex = jh_scan(nb, wsum, total) - nb;
        sc[tid] = bex;
        __syncthreads();
        const uint32_t b0 = bex - sc[lane0 > tile0 ? lane0 - tile0 : 0] + (lane0 < tile0 ? cblk : 0u);
        if (tid == JH_LANES - 1) bc[0] = b0 + nb;
        const int maxbegin = b0 > seg_nblk ? -1 : (int)(seg_nblk - b0);
        if (!active || maxbegin < 0) { nb = 0; ne = 0; }
        else if ((int)nb > maxbegin) {                           // the segment's blocks end inside this lane
            if ((int)nb == maxbegin + 1) { nb = (uint32_t)maxbegin; ne = nel; }
            else {
                p = ep; bi = ebk >> 8; k = ebk & 255u;
                jh_decode<false>(tabs, L, p, bi, k, maxbegin, nb, ne, nel, S);
            }
        }
        const uint32_t e0 = cent + jh_scan(ne, wsum, total) - ne;
        // ---- the storing pass ----
        if (active && maxbegin >= 0) {
            S.e = e0; S.blk = seg_blk0 + b0; S.bend = seg_blk0 + seg_nblk; S.err = 0;
            p = ep; bi = ebk >> 8; k = ebk & 255u;
            uint32_t wb, we, wl;
            jh_decode<true>(tabs, L, p, bi, k, maxbegin, wb, we, wl, S);
            if (lastlane && !S.err && !(S.blk == S.bend && k == 0)) S.err = JE_ENDS;
            if (S.err) atomicMin(status + blockIdx.x, (g + 1u) << 3 | S.err);
        }
        __syncthreads();
        cp = xp[JH_LANES - 1]; cbk = xs[JH_LANES - 1]; cblk = bc[0]; cent += total;
        __syncthreads();
    }
    if (tid == 0) S.tab[blocks] = cent;
}

// grid (images), 1024 threads: a lane per MCU, 1024 MCUs at a time
__global__ __launch_bounds__(JH_LANES) void k_jpeg_dc(uint32_t* __restrict__ s, const uint32_t* __restrict__ status)
{
    __shared__ uint32_t wv_v[3][16], wv_f[16];
    const uint32_t* hdr = s + (size_t)blockIdx.x * JPEG_HDR;
    const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6, ncomp = (int)hdr[0];
    const uint32_t blocks = hdr[4], cap = hdr[21];
    uint32_t* tab = s + hdr[5];
    uint32_t* ent = s + hdr[6];
    if (status[blockIdx.x] != JH_OK) {                           // refused: every block empty
        for (uint32_t i = tid; i <= blocks; i += JH_LANES) tab[i] = 0u;
        return;
    }
    const int hv = ncomp == 1 ? 1 : (int)(hdr[1] * hdr[2]), bpm = ncomp == 1 ? 1 : hv + 2;
    const uint32_t nm = blocks / (uint32_t)bpm, ri = hdr[24];
    uint32_t carry[3] = {0u, 0u, 0u};
    for (uint32_t m0 = 0; m0 < nm; m0 += JH_LANES) {
        const uint32_t m = m0 + tid;
        const bool active = m < nm;
        uint32_t f = active && m % ri == 0u ? 1u : 0u, v[3] = {0u, 0u, 0u}, d[4] = {0u, 0u, 0u, 0u}, at[6] = {cap, cap, cap, cap, cap, cap};
#pragma unroll
        for (int q = 0; q < 6; ++q)
            if (active && q < bpm) {
                const uint32_t e = tab[m * (uint32_t)bpm + q];
                at[q] = e < cap ? e : cap;
                const uint32_t x = e < cap ? ent[e] & 0xffffu : 0u;
                if (q < hv) { if (q < 4) d[q] = x; v[0] += x; }
                else if (q == hv) v[1] = x;
                else v[2] = x;
            }
        const uint32_t own[3] = {v[0], v[1], v[2]};
#pragma unroll
        for (int dd = 1; dd < 64; dd <<= 1) {                    // segmented inclusive scan inside the wave
            const uint32_t tf = __shfl_up(f, dd, 64);
            uint32_t tv[3];
#pragma unroll
            for (int c = 0; c < 3; ++c) tv[c] = __shfl_up(v[c], dd, 64);
            if (lane >= dd) {
                if (!f) { v[0] += tv[0]; v[1] += tv[1]; v[2] += tv[2]; }
                f |= tf;
            }
        }
        if (lane == 63) { wv_v[0][wv] = v[0]; wv_v[1][wv] = v[1]; wv_v[2][wv] = v[2]; wv_f[wv] = f; }
        __syncthreads();
        uint32_t in[3] = {carry[0], carry[1], carry[2]};
        for (int i = 0; i < 16; ++i) {
            if (i == wv && !f) { v[0] += in[0]; v[1] += in[1]; v[2] += in[2]; }
            const bool fl = wv_f[i] != 0u;
#pragma unroll
            for (int c = 0; c < 3; ++c) in[c] = fl ? wv_v[c][i] : in[c] + wv_v[c][i];
        }
        carry[0] = in[0]; carry[1] = in[1]; carry[2] = in[2];
        __syncthreads();
        uint32_t pred = v[0] - own[0];
#pragma unroll
        for (int q = 0; q < 6; ++q)
            if (active && q < bpm) {
                uint32_t x;
                if (q < hv) { if (q < 4) pred += d[q]; x = pred; }
                else x = q == hv ? v[1] : v[2];
                if (at[q] < cap) ent[at[q]] = x & 0xffffu;
            }
    }
}

// ---- host: the scan cut ----------------------------------------------------------------------------------------------------
struct JSeg { uint32_t off, len, blk0, nblk; };

static inline int jpeg_bpm(const JInfo& J) { return J.ncomp == 1 ? 1 : J.h[0] * J.v[0] + 2; }
static inline int jpeg_nseg(const JInfo& J) { const int nm = J.mcux * J.mcuy; return J.ri ? (nm + J.ri - 1) / J.ri : 1; }
static inline size_t jpeg_scan_bound(const JInfo& J, size_t n) { return ((n - J.scan + 3) & ~(size_t)3) + 4 * (size_t)jpeg_nseg(J); }

// One pass: the scan's bytes without the 00 after every FF, cut at the RSTn markers, every segment padded with zeros to 4 bytes.
// dst holds jpeg_scan_bound bytes and may be write-combined: it is written front to back and never read.
static bool cut_scan(const uint8_t* d, size_t n, const JInfo& J, uint8_t* dst, std::vector<JSeg>& segs, size_t& used, std::string& err)
{
    const int bpm = jpeg_bpm(J), nm = J.mcux * J.mcuy, ri = J.ri ? J.ri : nm, nseg = jpeg_nseg(J);
    size_t p = J.scan, o = 0;
    segs.clear();
    for (int sg = 0; sg < nseg; ++sg) {
        const size_t start = o;
        for (;;) {
            const uint8_t* q = p < n ? (const uint8_t*)memchr(d + p, 0xFF, n - p) : nullptr;
            const size_t run = (q ? (size_t)(q - d) : n) - p;
            memcpy(dst + o, d + p, run);
            o += run; p += run;
            if (q && p + 1 < n && d[p + 1] == 0) { dst[o++] = 0xFF; p += 2; continue; }
            break;                                               // a marker, or the data ends
        }
        const size_t len = o - start;
        while (o & 3) dst[o++] = 0;
        const int m0 = sg * ri, mn = nm - m0 < ri ? nm - m0 : ri;
        segs.push_back(JSeg{(uint32_t)start, (uint32_t)len, (uint32_t)(m0 * bpm), (uint32_t)(mn * bpm)});
        if (sg + 1 < nseg) {
            size_t q = p;
            while (q < n && d[q] == 0xFF) ++q;
            if (q >= n || q == p || d[q] != 0xD0 + (sg & 7)) return jfail(err, "bad restart marker");
            p = q + 1;
        }
    }
    used = o;
    return true;
}

static void jpeg_header_words(const JInfo& J, uint32_t* hdr)
{
    memset(hdr, 0, JPEG_HDR * sizeof(uint32_t));
    hdr[0] = J.ncomp; hdr[1] = J.h[0]; hdr[2] = J.v[0]; hdr[3] = J.mcux; hdr[4] = (uint32_t)(J.mcux * J.mcuy * jpeg_bpm(J));
    uint32_t off = 0;
    for (int c = 0; c < J.ncomp; ++c) {
        const uint32_t pitch = J.mcux * J.h[c] * 8, rows = J.mcuy * J.v[c] * 8;
        hdr[8 + c] = J.tq[c]; hdr[11 + c] = off; hdr[14 + c] = pitch;
        off += pitch * rows;
    }
    hdr[17] = (uint32_t)jpeg_nseg(J);
    hdr[24] = (uint32_t)(J.ri ? J.ri : J.mcux * J.mcuy);
    memcpy(hdr + 32, J.quant, sizeof J.quant);
}

// bytes == NULL: only the sizes (*bytes_used: the capacity to bring, *n_segments)
int ss_jpeg_scan_segments_impl(const unsigned char* data, size_t size, unsigned char* bytes, size_t bytes_cap, size_t* bytes_used, unsigned int* segments,
                               size_t seg_cap, int* n_segments, unsigned int* header, std::string& err)
{
    JInfo* J = new (std::nothrow) JInfo();
    if (!J) { err = "out of memory"; return SS_ERR_INVALID; }
    int rc = SS_ERR_INVALID;
    try {
        if (parse_headers(data, size, *J, err)) {
            const size_t bound = jpeg_scan_bound(*J, size);
            const int nseg = jpeg_nseg(*J);
            if (!bytes) { *bytes_used = bound; *n_segments = nseg; rc = SS_OK; }
            else if (bytes_cap < bound || seg_cap < (size_t)nseg) err = "buffers too small: " + std::to_string(bound) + " bytes and " + std::to_string(nseg) + " segments needed";
            else {
                std::vector<JSeg> segs;
                size_t used = 0;
                if (cut_scan(data, size, *J, bytes, segs, used, err)) {
                    for (int i = 0; i < nseg; ++i) { segments[4 * i] = segs[i].off; segments[4 * i + 1] = segs[i].len; segments[4 * i + 2] = segs[i].blk0; segments[4 * i + 3] = segs[i].nblk; }
                    *bytes_used = used; *n_segments = nseg;
                    if (header) jpeg_header_words(*J, header);
                    rc = SS_OK;
                }
            }
        }
    } catch (...) { err = "out of memory"; }
    delete J;
    return rc;
}

// ---- host: the batch call with the entropy stage on the device -------------------------------------------------------------
static int jpeg_slot_wait(SSJpeg::Slot& st, std::string& err)
{
    if (st.busy) {
        const hipError_t e = hipEventSynchronize(st.ev);
        st.busy = false;
        if (e != hipSuccess) { st.pending = 0; err = std::string("ss_jpeg_decode_batch: hipEventSynchronize: ") + hipGetErrorString(e); return SS_ERR_HIP; }
    }
    const int n = st.pending;
    st.pending = 0;
    const uint32_t* status = st.status_host.as<uint32_t>();
    for (int i = 0; i < n; ++i)
        if (status[i] != JH_OK) {
            const uint32_t code = status[i] & 7u;
            err = "ss_jpeg_decode_batch_device: image " + std::to_string(i) + ": " + kJpegCause[code < 7 ? code : 0];
            return SS_ERR_INVALID;
        }
    return SS_OK;
}

// ss_check_errors: the status words of device-entropy calls still in flight
int ss_jpeg_pending_impl(SSJpeg* j, std::string& err)
{
    if (!j) return SS_OK;
    int rc = SS_OK;
    for (auto& st : j->slot) {
        std::string e;
        const int r = jpeg_slot_wait(st, e);
        if (r != SS_OK && rc == SS_OK) { rc = r; err = e; }
    }
    return rc;
}

static void pack_huff(const JHuff& t, uint32_t* o)
{
    memset(o, 0, JH_TAB * sizeof(uint32_t));
    memcpy(o, t.fast, sizeof t.fast);
    for (int ln = 10; ln <= 16; ++ln) { o[256 + ln - 10] = (uint32_t)t.maxcode[ln]; o[264 + ln - 10] = (uint32_t)t.mincode[ln]; o[272 + ln - 10] = (uint32_t)t.valptr[ln]; }
    memcpy(o + 280, t.vals, sizeof t.vals);
}

struct JDevImage { JInfo J; std::vector<JSeg> segs; std::string err; bool ok = false; size_t at = 0, bound = 0, used = 0, tab_at = 0, ent_at = 0, rounds_at = 0, cap = 0, lanes = 0; };

// coef != NULL: the stage alone on one image (ss_jpeg_device_coefficients): no size check, no IDCT, the stream comes back and is expanded here.
int ss_jpeg_decode_device_impl(SSJpeg** state, hipStream_t stream, const unsigned char* const* data, const size_t* sizes, int n, int height, int width,
                               void* d_out, long long out_frame_stride, int rgb, int threads, short* coef, size_t coef_cap, std::string& err)
{
    try {
        if (!*state) *state = new SSJpeg();
        SSJpeg& S = **state;
        std::vector<JDevImage> img(n);
        const uint32_t W = (uint32_t)g_opt_jpeg_subseq_words;
        // ---- 1. headers ----
        auto heads = [&img, data, sizes, n, height, width, coef](int t, int nt) {
            for (int i = t; i < n; i += nt) {
                JDevImage& im = img[i];
                try {
                    if (!parse_headers(data[i], sizes[i], im.J, im.err)) continue;
                    if (!coef && (im.J.width != width || im.J.height != height)) {
                        im.err = "size " + std::to_string(im.J.width) + "x" + std::to_string(im.J.height) + " differs from the batch's " + std::to_string(width) + "x" + std::to_string(height);
                        continue;
                    }
                    im.bound = jpeg_scan_bound(im.J, sizes[i]);
                    im.ok = true;
                } catch (...) { im.err = "out of memory"; }
            }
        };
        const int T = threads < n ? threads : n;
        if (!run_threads(T, heads)) { err = "ss_jpeg_decode_batch_device: host stage failed"; return SS_ERR_INVALID; }
        for (int i = 0; i < n; ++i)
            if (!img[i].ok) { err = "ss_jpeg_decode_batch_device: image " + std::to_string(i) + ": " + img[i].err; return SS_ERR_INVALID; }
        // ---- 2. layout of what crosses PCIe: headers, then per image its Huffman tables, segment table and scan bytes ----
        size_t at = (size_t)n * JPEG_HDR;
        for (int i = 0; i < n; ++i) {
            JDevImage& im = img[i];
            im.at = at;
            at += (size_t)im.J.ncomp * 2 * JH_TAB + (size_t)jpeg_nseg(im.J) * JH_SEG + im.bound / 4;
        }
        if (at >= ((size_t)1 << 30)) { err = "ss_jpeg_decode_batch_device: scans beyond 4 GiB"; return SS_ERR_CAPACITY; }
        const size_t in_words = at;
        SSJpeg::Slot& st = S.slot[S.next];
        if (int rcw = jpeg_slot_wait(st, err)) return rcw;
        SS_HIPCHK(kJpegWho, st.ev.ensure());
        SS_HIPCHK(kJpegWho, st.status_dev.reserve(64 * sizeof(uint32_t), SS_EXACT));
        SS_HIPCHK(kJpegWho, st.status_host.reserve(64 * sizeof(uint32_t), SS_EXACT));
        if (int rcr = jpeg_slot_reserve(st, in_words * 4, 0, 0, err)) return rcr;       // (the device's share is known after the cut)
        // ---- 3. the scan cut and the tables, straight into the staging area ----
        uint32_t* base = st.host.as<uint32_t>();
        auto cut = [&img, base, data, sizes, n, W](int t, int nt) {
            for (int i = t; i < n; i += nt) {
                JDevImage& im = img[i];
                im.ok = false;
                try {
                    const JInfo& J = im.J;
                    uint32_t* o = base + im.at;
                    uint32_t tb[JH_TAB];
                    for (int c = 0; c < J.ncomp; ++c) {
                        pack_huff(J.dc[J.td[c]], tb); memcpy(o, tb, sizeof tb); o += JH_TAB;
                        pack_huff(J.ac[J.ta[c]], tb); memcpy(o, tb, sizeof tb); o += JH_TAB;
                    }
                    const size_t nseg = (size_t)jpeg_nseg(J);
                    if (!cut_scan(data[i], sizes[i], J, (uint8_t*)(o + nseg * JH_SEG), im.segs, im.used, im.err)) continue;
                    std::vector<uint32_t> rec(nseg * JH_SEG);
                    size_t lanes = 0, bytes = 0;
                    for (size_t k = 0; k < nseg; ++k) {
                        const JSeg& sg = im.segs[k];
                        rec[k * JH_SEG] = sg.off; rec[k * JH_SEG + 1] = sg.len; rec[k * JH_SEG + 2] = sg.blk0; rec[k * JH_SEG + 3] = sg.nblk; rec[k * JH_SEG + 4] = (uint32_t)lanes;
                        const size_t sub = ((size_t)sg.len + 4 * W - 1) / (4 * W);
                        lanes += sub ? sub : 1;
                        bytes += sg.len;
                    }
                    memcpy(o, rec.data(), rec.size() * 4);
                    im.lanes = lanes;
                    im.cap = (size_t)J.mcux * J.mcuy * jpeg_bpm(J) + 4 * bytes;
                    im.ok = true;
                } catch (...) { im.err = "out of memory"; }
            }
        };
        if (!run_threads(T, cut)) { err = "ss_jpeg_decode_batch_device: host stage failed"; return SS_ERR_INVALID; }
        for (int i = 0; i < n; ++i)
            if (!img[i].ok) { err = "ss_jpeg_decode_batch_device: image " + std::to_string(i) + ": " + img[i].err; return SS_ERR_INVALID; }
        // ---- 4. layout of what stays on the device: block tables (zeroed), rounds, entries; then the headers ----
        int max_blk = 0;
        const size_t tabs_at = at;
        for (int i = 0; i < n; ++i) { img[i].tab_at = at; at += (size_t)img[i].J.mcux * img[i].J.mcuy * jpeg_bpm(img[i].J) + 1; }
        const size_t tabs_words = at - tabs_at;
        for (int i = 0; i < n; ++i) { img[i].rounds_at = at; at += (img[i].lanes + JH_LANES - 1) / JH_LANES; }
        for (int i = 0; i < n; ++i) { img[i].ent_at = at; at += img[i].cap; }
        if (at >= ((size_t)1 << 32)) { err = "ss_jpeg_decode_batch_device: coefficient stream beyond 2^32 entries"; return SS_ERR_CAPACITY; }
        for (int i = 0; i < n; ++i) {
            const JDevImage& im = img[i];
            uint32_t hdr[JPEG_HDR];
            jpeg_header_words(im.J, hdr);
            if ((int)hdr[4] > max_blk) max_blk = (int)hdr[4];
            hdr[5] = (uint32_t)im.tab_at; hdr[6] = (uint32_t)im.ent_at;
            hdr[19] = (uint32_t)im.at;
            hdr[25] = hdr[19] + (uint32_t)im.J.ncomp * 2 * JH_TAB;
            hdr[18] = hdr[25] + hdr[17] * JH_SEG;
            hdr[20] = (uint32_t)im.lanes; hdr[21] = (uint32_t)im.cap; hdr[22] = (uint32_t)im.rounds_at; hdr[23] = W;
            memcpy(base + (size_t)i * JPEG_HDR, hdr, sizeof hdr);
        }
        const size_t bytes = at * 4;
        const size_t plane_slot = 3 * (size_t)((width + 15) / 16 * 16) * ((height + 15) / 16 * 16), planes_bytes = coef ? 0 : plane_slot * n;
        if (int rcr = jpeg_slot_reserve(st, in_words * 4, bytes, planes_bytes, err)) return rcr;
        uint32_t* dev = st.dev.as<uint32_t>();
        uint32_t* status = st.status_dev.as<uint32_t>();
        uint8_t* planes = st.planes.as<uint8_t>();
        // ---- 5. one copy, the two entropy kernels, the two kernels of the host stage's path, the status ----
        SS_HIPCHK(kJpegWho, hipMemcpyAsync(dev, base, in_words * 4, hipMemcpyHostToDevice, stream));
        SS_HIPCHK(kJpegWho, hipMemsetAsync(dev + tabs_at, 0, tabs_words * 4, stream));
        SS_HIPCHK(kJpegWho, hipMemsetAsync(status, 0xff, (size_t)n * 4, stream));
        hipLaunchKernelGGL(k_jpeg_huff, dim3(n), dim3(JH_LANES), 0, stream, dev, status);
        hipLaunchKernelGGL(k_jpeg_dc, dim3(n), dim3(JH_LANES), 0, stream, dev, status);
        if (!coef) {
            hipLaunchKernelGGL(k_jpeg_idct, dim3((max_blk + 31) / 32, n), dim3(256), 0, stream, dev, planes, (long long)plane_slot);
            const int groups = (height * width + 3) / 4;
            const int dwords = (((uintptr_t)d_out | (uintptr_t)out_frame_stride) & 3) == 0;
            hipLaunchKernelGGL(k_jpeg_pixels, dim3((groups + 255) / 256, n), dim3(256), 0, stream, dev, planes, (long long)plane_slot, height, width,
                               (uint8_t*)d_out, out_frame_stride, rgb, dwords);
        }
        SS_HIPCHK(kJpegWho, hipGetLastError());
        SS_HIPCHK(kJpegWho, hipMemcpyAsync(st.status_host.as(), status, (size_t)n * 4, hipMemcpyDeviceToHost, stream));
        SS_HIPCHK(kJpegWho, hipEventRecord(st.ev, stream));
        st.busy = true;
        st.pending = n;
        S.next ^= 1;
        if (!coef) return SS_OK;
        // ---- the stage alone: wait, read the stream back, expand ----
        if (int rcw = jpeg_slot_wait(st, err)) return rcw;
        const JDevImage& im = img[0];
        const JInfo& J = im.J;
        const size_t blocks = (size_t)J.mcux * J.mcuy * jpeg_bpm(J), tiles = (im.lanes + JH_LANES - 1) / JH_LANES;
        size_t cbase[3] = {0, 0, 0}, tot = 0;
        for (int c = 0; c < J.ncomp; ++c) { cbase[c] = tot; tot += (size_t)J.mcux * J.h[c] * J.mcuy * J.v[c] * 64; }
        if (tot > coef_cap) { err = "coefficient buffer too small: " + std::to_string(tot) + " values needed"; return SS_ERR_INVALID; }
        std::vector<uint32_t> tab(blocks + 1), rnd(tiles);
        SS_HIPCHK(kJpegWho, hipMemcpy(tab.data(), dev + im.tab_at, tab.size() * 4, hipMemcpyDeviceToHost));
        SS_HIPCHK(kJpegWho, hipMemcpy(rnd.data(), dev + im.rounds_at, rnd.size() * 4, hipMemcpyDeviceToHost));
        const size_t ne = tab[blocks];
        if (ne > im.cap) { err = "ss_jpeg_device_coefficients: entry total beyond the capacity"; return SS_ERR_INVALID; }
        std::vector<uint32_t> ent(ne ? ne : 1);
        if (ne) SS_HIPCHK(kJpegWho, hipMemcpy(ent.data(), dev + im.ent_at, ne * 4, hipMemcpyDeviceToHost));
        S.rounds.assign(rnd.begin(), rnd.end());
        memset(coef, 0, tot * sizeof(short));
        const int bpm = jpeg_bpm(J), hv = J.ncomp == 1 ? 1 : J.h[0] * J.v[0];
        for (size_t b = 0; b < blocks; ++b) {
            const size_t m = b / bpm;
            const int jj = (int)(b % bpm), my = (int)(m / J.mcux), mx = (int)(m % J.mcux);
            int c = 0, by = my, bx = mx;
            if (jj < hv) { by = my * J.v[0] + jj / J.h[0]; bx = mx * J.h[0] + jj % J.h[0]; }
            else c = 1 + jj - hv;
            short* o = coef + cbase[c] + ((size_t)by * (J.mcux * J.h[c]) + bx) * 64;
            if (tab[b] > tab[b + 1] || tab[b + 1] > ne) { err = "ss_jpeg_device_coefficients: block table out of order"; return SS_ERR_INVALID; }
            for (size_t e = tab[b]; e < tab[b + 1]; ++e) o[(ent[e] >> 16) & 63u] = (short)(uint16_t)(ent[e] & 0xffffu);
        }
        return SS_OK;
    } catch (...) {
        err = "ss_jpeg_decode_batch_device: out of memory";
        return SS_ERR_INVALID;
    }
}

int ss_jpeg_device_rounds_impl(SSJpeg* j, int* rounds, int cap)
{
    if (!j) return 0;
    const int n = (int)j->rounds.size();
    for (int i = 0; i < n && i < cap; ++i) rounds[i] = j->rounds[i];
    return n;
}
