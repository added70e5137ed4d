// ss_jpeg_enc.hip — frames on the device written as baseline JPEG files (docs/JPEG.md "Encoding"): the mirror of ss_jpeg.hip.
//
// Two kernels do everything that is independent per 8x8 block, for all images of the call at once:
//   k_jpegenc_fdct  eight lanes per block: gather the block's 64 samples from the HWC frame (colour conversion and chroma
//                   downsampling on the fly, clamped indices), ISLOW forward DCT (pass 1 on the lane's row in registers, pass 2 on
//                   its column through LDS), quantisation, the 64 values in zig-zag order as int16 into a dense device-only
//                   buffer, the block's non-zero count into a table in SCAN order
//   k_jpegenc_pack  exclusive scan of the counts per image, then the compaction: a wave per block, a lane per coefficient
// What crosses to the host is the SPARSE stream (a 32-bit offset per block, a 32-bit entry per non-zero coefficient).  The serial
// part, Huffman coding with the Annex K tables, runs on the call's host threads, whole images per thread.
// Every value is an integer; the files equal libjpeg-turbo's defaults (JDCT_ISLOW, standard tables) byte for byte.
//
// ss_jpeg_encode_batch_device (docs/JPEG.md section 13) keeps the entropy stage on the device as well: from k_jpegenc_fdct's dense blocks
//   k_jpegenc_hlen   a wave per block: the block's bit length (DC difference against the nearest earlier real block of its component)
//   k_jpegenc_hwrite exclusive scan of the lengths per image (64-bit positions), every block's bits ORed into the zeroed unstuffed stream
//   k_jpegenc_ffcount / k_jpegenc_stuff   the FF bytes counted per chunk, then every byte moved to its place with a 00 behind each FF
// and only the files' own bytes cross to the host.
#include <cstring>
#include <string>
#include <vector>
#include "ss_common.h"
#include "ss_host.h"
#include "ss_launch.h"
#include "ss_jpeg_host.h"

#define JENC_WS_PITCH 72                // LDS dwords per block, rows of 9 (8 + 1 pad), as in k_jpeg_idct
#define JENC_PACK_THREADS 1024
#define JENC_HEADER_BYTES 625           // SOI, APP0, 2 DQT, SOF0, 4 DHT, SOS, EOI
#define JENC_BLOCK_BYTES 416            // 20 bits of DC + 63 * 26 bits of AC = 208 bytes, every one of them stuffed

// ---- tables ----------------------------------------------------------------------------------------------------------------
// Annex K.1 / K.2, natural order
static const uint8_t kBaseQuant[2][64] = {
    {16, 11, 10, 16, 24, 40, 51, 61, 12, 12, 14, 19, 26, 58, 60, 55, 14, 13, 16, 24, 40, 57, 69, 56, 14, 17, 22, 29, 51, 87, 80, 62,
     18, 22, 37, 56, 68, 109, 103, 77, 24, 35, 55, 64, 81, 104, 113, 92, 49, 64, 78, 87, 103, 121, 120, 101, 72, 92, 95, 98, 112, 100, 103, 99},
    {17, 18, 24, 47, 99, 99, 99, 99, 18, 21, 26, 66, 99, 99, 99, 99, 24, 26, 56, 99, 99, 99, 99, 99, 47, 66, 99, 99, 99, 99, 99, 99,
     99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99}};

// Annex K.3.3 - K.3.6: code counts per length 1 .. 16, then the symbols; order DC 0, AC 0, DC 1, AC 1 (the order of the DHT segments)
static const uint8_t kDcCounts[2][16] = {{0, 1, 5, 1, 1, 1, 1, 1, 1, 0, 0, 0, 0, 0, 0, 0}, {0, 3, 1, 1, 1, 1, 1, 1, 1, 1, 1, 0, 0, 0, 0, 0}};
static const uint8_t kDcSyms[12] = {0, 1, 2, 3, 4, 5, 6, 7, 8, 9, 10, 11};
static const uint8_t kAcCounts[2][16] = {{0, 2, 1, 3, 3, 2, 4, 3, 5, 5, 4, 4, 0, 0, 1, 125}, {0, 2, 1, 2, 4, 4, 3, 4, 7, 5, 4, 4, 0, 1, 2, 119}};
static const uint8_t kAcSyms[2][162] = {
    {1, 2, 3, 0, 4, 17, 5, 18, 33, 49, 65, 6, 19, 81, 97, 7, 34, 113, 20, 50, 129, 145, 161, 8, 35, 66, 177, 193, 21, 82, 209, 240, 36, 51, 98, 114, 130, 9, 10,
     22, 23, 24, 25, 26, 37, 38, 39, 40, 41, 42, 52, 53, 54, 55, 56, 57, 58, 67, 68, 69, 70, 71, 72, 73, 74, 83, 84, 85, 86, 87, 88, 89, 90, 99, 100, 101, 102,
     103, 104, 105, 106, 115, 116, 117, 118, 119, 120, 121, 122, 131, 132, 133, 134, 135, 136, 137, 138, 146, 147, 148, 149, 150, 151, 152, 153, 154, 162, 163,
     164, 165, 166, 167, 168, 169, 170, 178, 179, 180, 181, 182, 183, 184, 185, 186, 194, 195, 196, 197, 198, 199, 200, 201, 202, 210, 211, 212, 213, 214, 215,
     216, 217, 218, 225, 226, 227, 228, 229, 230, 231, 232, 233, 234, 241, 242, 243, 244, 245, 246, 247, 248, 249, 250},
    {0, 1, 2, 3, 17, 4, 5, 33, 49, 6, 18, 65, 81, 7, 97, 113, 19, 34, 50, 129, 8, 20, 66, 145, 161, 177, 193, 9, 35, 51, 82, 240, 21, 98, 114, 209, 10, 22, 36,
     52, 225, 37, 241, 23, 24, 25, 26, 38, 39, 40, 41, 42, 53, 54, 55, 56, 57, 58, 67, 68, 69, 70, 71, 72, 73, 74, 83, 84, 85, 86, 87, 88, 89, 90, 99, 100, 101,
     102, 103, 104, 105, 106, 115, 116, 117, 118, 119, 120, 121, 122, 130, 131, 132, 133, 134, 135, 136, 137, 138, 146, 147, 148, 149, 150, 151, 152, 153, 154,
     162, 163, 164, 165, 166, 167, 168, 169, 170, 178, 179, 180, 181, 182, 183, 184, 185, 186, 194, 195, 196, 197, 198, 199, 200, 201, 202, 210, 211, 212, 213,
     214, 215, 216, 217, 218, 226, 227, 228, 229, 230, 231, 232, 233, 234, 242, 243, 244, 245, 246, 247, 248, 249, 250}};

// q[k] = clamp((base[k] * s + 50) / 100, 1, 255) with s = 5000 / Q below 50 and 200 - 2 Q from there; natural order, [0] luma [1] chroma
static void jenc_quant(int quality, uint16_t (&q)[2][64])
{
    const int s = quality < 50 ? 5000 / quality : 200 - 2 * quality;
    for (int t = 0; t < 2; ++t)
        for (int k = 0; k < 64; ++k) {
            const int v = (kBaseQuant[t][k] * s + 50) / 100;
            q[t][k] = (uint16_t)(v < 1 ? 1 : v > 255 ? 255 : v);
        }
}

// ---- host: the entropy stage -----------------------------------------------------------------------------------------------
struct JEncHuff { uint16_t code[256]; uint8_t len[256]; };      // len 0: the table has no such symbol

static void jenc_build(JEncHuff& t, const uint8_t* counts, const uint8_t* syms)
{
    memset(&t, 0, sizeof t);
    int code = 0, k = 0;
    for (int ln = 1; ln <= 16; ++ln) {
        for (int i = 0; i < counts[ln - 1]; ++i, ++code, ++k) { t.code[syms[k]] = (uint16_t)code; t.len[syms[k]] = (uint8_t)ln; }
        code <<= 1;
    }
}

struct JEncTables {
    JEncHuff dc[2], ac[2];
    JEncTables() { for (int t = 0; t < 2; ++t) { jenc_build(dc[t], kDcCounts[t], kDcSyms); jenc_build(ac[t], kAcCounts[t], kAcSyms[t]); } }
};
static const JEncTables kEnc;

struct JEncBits {
    uint8_t* p;
    uint64_t acc = 0;
    int n = 0;                          // bits waiting in acc (below 32 between calls)
    inline void bytes(int k)
    {
        for (; k > 0; --k, n -= 8) {
            const uint8_t b = (uint8_t)(acc >> (n - 8));
            *p++ = b;
            if (b == 0xFF) *p++ = 0;
        }
    }
    inline void put(uint32_t bits, int len)                         // len <= 27
    {
        acc = (acc << len) | bits;
        n += len;
        if (n >= 32) {
            uint32_t w = (uint32_t)(acc >> (n - 32));
            const uint32_t x = ~w;
            if (!((x - 0x01010101u) & ~x & 0x80808080u)) {          // four bytes without an FF: stored at once
                w = __builtin_bswap32(w);
                memcpy(p, &w, 4);
                p += 4;
                n -= 32;
            } else bytes(4);
        }
    }
    inline void finish()                                            // the last byte is padded with 1-bits
    {
        bytes(n >> 3);
        if (n) { acc = (acc << (8 - n)) | ((1u << (8 - n)) - 1); n = 8; bytes(1); }
    }
};

static inline int jenc_category(int v) { return v ? 32 - __builtin_clz((unsigned)(v < 0 ? -v : v)) : 0; }

// One block: its non-zero coefficients as entries (zig-zag index << 16 | uint16 value) in rising zig-zag order
static inline bool jenc_block(JEncBits& b, const uint32_t* ent, int cnt, int& pred, const JEncHuff& dc, const JEncHuff& ac)
{
    int i = 0, v = 0;
    if (cnt && (ent[0] >> 16) == 0) { v = (int16_t)(ent[0] & 0xffffu); i = 1; }
    const int diff = v - pred;
    pred = v;
    int s = jenc_category(diff);
    if (s > 11) return false;
    b.put(((uint32_t)dc.code[s] << s) | ((uint32_t)(diff < 0 ? diff - 1 : diff) & ((1u << s) - 1)), dc.len[s] + s);
    int k = 1;                                                      // the next zig-zag index to be coded
    for (; i < cnt; ++i) {
        const int zz = (int)(ent[i] >> 16);
        v = (int16_t)(ent[i] & 0xffffu);
        int run = zz - k;
        if (run < 0 || zz > 63) return false;
        for (; run > 15; run -= 16) b.put(ac.code[0xF0], ac.len[0xF0]);
        s = jenc_category(v);
        if (s > 10) return false;
        const int sym = (run << 4) | s;
        b.put(((uint32_t)ac.code[sym] << s) | ((uint32_t)(v < 0 ? v - 1 : v) & ((1u << s) - 1)), ac.len[sym] + s);
        k = zz + 1;
    }
    if (k < 64) b.put(ac.code[0], ac.len[0]);
    return true;
}

// A dummy block (outside the component's real blocks): all AC zero, the DC of the block before it, so its difference is 0
static inline void jenc_dummy(JEncBits& b, const JEncHuff& dc, const JEncHuff& ac)
{
    b.put(dc.code[0], dc.len[0]);
    b.put(ac.code[0], ac.len[0]);
}

struct JEncShape {
    int W, H, hm, vm, mcux, mcuy, bpm, nscan;
    int bw[2], bh[2];                   // real blocks of luma [0] and of a chroma component [1]
    JEncShape(int width, int height, int h, int v) : W(width), H(height), hm(h), vm(v)
    {
        mcux = (W + 8 * hm - 1) / (8 * hm);
        mcuy = (H + 8 * vm - 1) / (8 * vm);
        bpm = hm * vm + 2;
        nscan = mcux * mcuy * bpm;
        bw[0] = (W + 7) / 8; bh[0] = (H + 7) / 8;
        bw[1] = ((W + hm - 1) / hm + 7) / 8; bh[1] = ((H + vm - 1) / vm + 7) / 8;
    }
};

size_t ss_jpeg_encode_bound_impl(int width, int height, int h_samp, int v_samp)
{
    const JEncShape S(width, height, h_samp, v_samp);
    return JENC_HEADER_BYTES + 15 + (size_t)S.nscan * JENC_BLOCK_BYTES;
}

static uint8_t* jenc_header(uint8_t* p, const JEncShape& S, const uint16_t (&q)[2][64])
{
    auto put16 = [&p](int v) { *p++ = (uint8_t)(v >> 8); *p++ = (uint8_t)v; };
    put16(0xFFD8);
    put16(0xFFE0); put16(16); memcpy(p, "JFIF\0\1\1\0\0\1\0\1\0\0", 14); p += 14;
    for (int t = 0; t < 2; ++t) {
        put16(0xFFDB); put16(67); *p++ = (uint8_t)t;
        for (int k = 0; k < 64; ++k) *p++ = (uint8_t)q[t][kZigzag[k]];
    }
    put16(0xFFC0); put16(17); *p++ = 8; put16(S.H); put16(S.W); *p++ = 3;
    *p++ = 1; *p++ = (uint8_t)(S.hm << 4 | S.vm); *p++ = 0;
    *p++ = 2; *p++ = 0x11; *p++ = 1;
    *p++ = 3; *p++ = 0x11; *p++ = 1;
    for (int t = 0; t < 2; ++t) {
        put16(0xFFC4); put16(31); *p++ = (uint8_t)t; memcpy(p, kDcCounts[t], 16); p += 16; memcpy(p, kDcSyms, 12); p += 12;
        put16(0xFFC4); put16(181); *p++ = (uint8_t)(0x10 | t); memcpy(p, kAcCounts[t], 16); p += 16; memcpy(p, kAcSyms[t], 162); p += 162;
    }
    put16(0xFFDA); put16(12); *p++ = 3; *p++ = 1; *p++ = 0x00; *p++ = 2; *p++ = 0x11; *p++ = 3; *p++ = 0x11; *p++ = 0; *p++ = 63; *p++ = 0;
    return p;
}

// The whole file of one image.  Block(s, comp, by, bx, ent) -> the entry count of the real block at scan position s, its entries in ent
// (a pointer it may redirect).  out holds at least ss_jpeg_encode_bound bytes.
template <class Block>
static bool jenc_file(const JEncShape& S, const uint16_t (&q)[2][64], Block block, uint8_t* out, size_t* out_size)
{
    JEncBits b{jenc_header(out, S, q)};
    int pred[3] = {0, 0, 0};
    int s = 0;
    for (int my = 0; my < S.mcuy; ++my)
        for (int mx = 0; mx < S.mcux; ++mx)
            for (int j = 0; j < S.bpm; ++j, ++s) {
                const int comp = j < S.hm * S.vm ? 0 : 1 + j - S.hm * S.vm, t = comp ? 1 : 0;
                const int by = comp ? my : my * S.vm + j / S.hm, bx = comp ? mx : mx * S.hm + j % S.hm;
                if (by >= S.bh[t] || bx >= S.bw[t]) { jenc_dummy(b, kEnc.dc[t], kEnc.ac[t]); continue; }
                uint32_t tmp[64];
                const uint32_t* ent = tmp;
                const int cnt = block(s, comp, by, bx, tmp, ent);
                if (!jenc_block(b, ent, cnt, pred[comp], kEnc.dc[t], kEnc.ac[t])) return false;
            }
    b.finish();
    *b.p++ = 0xFF; *b.p++ = 0xD9;
    *out_size = (size_t)(b.p - out);
    return true;
}

// The arguments have been checked (ss_api.hip)
int ss_jpeg_entropy_encode_impl(const short* coef, int quality, int width, int height, int h_samp, int v_samp, unsigned char* out, size_t* out_size,
                                std::string& err)
{
    const JEncShape S(width, height, h_samp, v_samp);
    uint16_t q[2][64];
    jenc_quant(quality, q);
    // ss_jpeg_coefficients' layout: component after component, each one's blocks in raster order over its whole-MCU grid
    const size_t ybl = (size_t)S.mcux * S.hm * S.mcuy * S.vm, cbl = (size_t)S.mcux * S.mcuy;
    auto block = [&](int, int comp, int by, int bx, uint32_t* tmp, const uint32_t*&) {
        const short* c = coef + (comp == 0 ? ((size_t)by * S.mcux * S.hm + bx) : ybl + (comp - 1) * cbl + (size_t)by * S.mcux + bx) * 64;
        int n = 0;
        for (int k = 0; k < 64; ++k)
            if (c[kZigzag[k]]) tmp[n++] = (uint32_t)k << 16 | (uint16_t)c[kZigzag[k]];
        return n;
    };
    if (!jenc_file(S, q, block, out, out_size)) { err = "a coefficient beyond the baseline categories (DC difference 11 bits, AC 10 bits)"; return SS_ERR_INVALID; }
    return SS_OK;
}

// ---- device ----------------------------------------------------------------------------------------------------------------
struct JEncParams {
    uint16_t q[2][64];                  // natural order
    uint32_t recip[2][64];              // floor(2^32 / (8 q)) + 1: (a * recip) >> 32 == a / (8 q) for every a the transform can give (tests/test_jpeg_encode_cpu.py)
    uint8_t zz[64];                     // natural index -> zig-zag position
};

// One 1-D pass of jfdctint's ISLOW on d[0..7] (docs/JPEG.md "Encoding"); int32 with wrap-around like the decoder's passes
template <bool FIRST>
__device__ __forceinline__ void jenc_pass(uint32_t (&d)[8])
{
    constexpr int s = FIRST ? 11 : 15;
    constexpr uint32_t r = 1u << (s - 1);
    const uint32_t t0 = d[0] + d[7], t7 = d[0] - d[7], t1 = d[1] + d[6], t6 = d[1] - d[6], t2 = d[2] + d[5], t5 = d[2] - d[5], t3 = d[3] + d[4], t4 = d[3] - d[4];
    const uint32_t t10 = t0 + t3, t13 = t0 - t3, t11 = t1 + t2, t12 = t1 - t2;
    if (FIRST) { d[0] = (t10 + t11) << 2; d[4] = (t10 - t11) << 2; }
    else { d[0] = (uint32_t)((int32_t)(t10 + t11 + 2u) >> 2); d[4] = (uint32_t)((int32_t)(t10 - t11 + 2u) >> 2); }
    uint32_t z1 = (t12 + t13) * 4433u;
    d[2] = (uint32_t)((int32_t)(z1 + t13 * 6270u + r) >> s);
    d[6] = (uint32_t)((int32_t)(z1 - t12 * 15137u + r) >> s);
    z1 = t4 + t7;
    uint32_t z2 = t5 + t6, z3 = t4 + t6, z4 = t5 + t7;
    const uint32_t z5 = (z3 + z4) * 9633u;
    const uint32_t u4 = t4 * 2446u, u5 = t5 * 16819u, u6 = t6 * 25172u, u7 = t7 * 12299u;
    z1 = 0u - z1 * 7373u; z2 = 0u - z2 * 20995u; z3 = z5 - z3 * 16069u; z4 = z5 - z4 * 3196u;
    d[7] = (uint32_t)((int32_t)(u4 + z1 + z3 + r) >> s);
    d[5] = (uint32_t)((int32_t)(u5 + z2 + z4 + r) >> s);
    d[3] = (uint32_t)((int32_t)(u6 + z2 + z3 + r) >> s);
    d[1] = (uint32_t)((int32_t)(u7 + z1 + z4 + r) >> s);
}

// grid (ceil(scan positions / 32), images), 256 threads: 8 lanes per block, 32 blocks per workgroup.  A block is named by its scan
// position (MCU after MCU; inside an MCU the hm * vm luma blocks row by row, then Cb, then Cr); positions outside the component's real
// blocks (the dummies that complete an MCU) only write a count of 0.
__global__ __launch_bounds__(256) void k_jpegenc_fdct(const uint8_t* __restrict__ in, long long in_stride, int H, int W, int rgb, int hm, int vm, int mcux,
                                                      int nscan, int16_t* __restrict__ dense, uint32_t* __restrict__ cnt, uint32_t* __restrict__ totals,
                                                      const JEncParams P)
{
    __shared__ uint32_t ws[32 * JENC_WS_PITCH];
    const int img = blockIdx.y, lb = threadIdx.x >> 3, l = threadIdx.x & 7, s = blockIdx.x * 32 + lb;
    uint32_t* w = ws + lb * JENC_WS_PITCH;
    const int bpm = hm * vm + 2, mcu = s / bpm, jj = s - mcu * bpm, my = mcu / mcux, mx = mcu - my * mcux;
    int comp = 0, by = my, bx = mx;
    if (jj < hm * vm) { by = my * vm + jj / hm; bx = mx * hm + jj % hm; }
    else comp = 1 + jj - hm * vm;
    const int cw = comp ? (W + hm - 1) / hm : W, ch = comp ? (H + vm - 1) / vm : H;        // the component's plane
    const bool on = s < nscan && by * 8 < ch && bx * 8 < cw;
    const uint8_t* src = in + (size_t)img * in_stride;
    const int ir = rgb ? 0 : 2, ib = 2 - ir;
    uint32_t x[8];
#pragma unroll
    for (int i = 0; i < 8; ++i) x[i] = 0u;
    if (on && comp == 0) {
        const uint8_t* row = src + (size_t)min(by * 8 + l, H - 1) * W * 3;
#pragma unroll
        for (int i = 0; i < 8; ++i) {
            const uint8_t* p = row + min(bx * 8 + i, W - 1) * 3;
            x[i] = (uint32_t)(((19595 * p[ir] + 38470 * p[1] + 7471 * p[ib] + 32768) >> 16) - 128);
        }
    } else if (on) {
        // chroma sample (cy, cx): vertically the DOWNSAMPLED last row is replicated (cy clamped), horizontally the full-size last
        // column (cx is not clamped, the pixel columns are); the rounding bias alternates with cx, in the padded columns too
        const int kr = comp == 1 ? -11059 : 32768, kg = comp == 1 ? -21709 : -27439, kb = comp == 1 ? 32768 : -5329;
        const int cy = min(by * 8 + l, ch - 1);
        const uint8_t* row0 = src + (size_t)min(vm * cy, H - 1) * W * 3;
        const uint8_t* row1 = src + (size_t)min(vm * cy + vm - 1, H - 1) * W * 3;
        auto chroma = [=](const uint8_t* p) { return (kr * p[ir] + kg * p[1] + kb * p[ib] + 8388608 + 32767) >> 16; };
#pragma unroll
        for (int i = 0; i < 8; ++i) {
            const int cx = bx * 8 + i, x0 = min(hm * cx, W - 1) * 3, x1 = min(hm * cx + hm - 1, W - 1) * 3;
            int v = chroma(row0 + x0);
            if (hm == 2) {
                v += chroma(row0 + x1);
                if (vm == 2) v = (v + chroma(row1 + x0) + chroma(row1 + x1) + 1 + (cx & 1)) >> 2;
                else v = (v + (cx & 1)) >> 1;
            }
            x[i] = (uint32_t)(v - 128);
        }
    }
    jenc_pass<true>(x);                                          // the lane's row
#pragma unroll
    for (int i = 0; i < 8; ++i) w[l * 9 + i] = x[i];
    __syncthreads();
#pragma unroll
    for (int i = 0; i < 8; ++i) x[i] = w[i * 9 + l];             // lane = column
    jenc_pass<false>(x);
    __syncthreads();
    const int t = comp ? 1 : 0;
#pragma unroll
    for (int i = 0; i < 8; ++i) {                                // x[i] is coefficient (row i, column l), 8 x its true value
        const int k = i * 8 + l, c = (int32_t)x[i];
        const uint32_t qv = (uint32_t)P.q[t][k] << 3, a = (uint32_t)(c < 0 ? -c : c) + (qv >> 1);
        const int m = (int)__umulhi(a, P.recip[t][k]);
        const int z = P.zz[k];
        w[(z >> 3) * 9 + (z & 7)] = (uint32_t)(c < 0 ? -m : m);
    }
    __syncthreads();
    uint32_t v[8];
    int c = 0;
#pragma unroll
    for (int i = 0; i < 8; ++i) { v[i] = w[l * 9 + i]; c += v[i] != 0u; }
    c += __shfl_xor(c, 1); c += __shfl_xor(c, 2); c += __shfl_xor(c, 4);                  // the block's count, in its eight lanes
    if (on) {
        uint4 o;
        o.x = (v[0] & 0xffffu) | v[1] << 16; o.y = (v[2] & 0xffffu) | v[3] << 16; o.z = (v[4] & 0xffffu) | v[5] << 16; o.w = (v[6] & 0xffffu) | v[7] << 16;
        *(uint4*)(dense + ((size_t)img * nscan + s) * 64 + l * 8) = o;
    }
    if (l == 0 && s < nscan) cnt[(size_t)img * nscan + s] = (uint32_t)c;                  // (a block that is not `on` transformed zeros: 0)
    int tot = l == 0 ? c : 0;                                    // one atomic per wave for the image's entry total
    tot += __shfl_xor(tot, 8); tot += __shfl_xor(tot, 16); tot += __shfl_xor(tot, 32);
    if ((threadIdx.x & 63) == 0 && tot) atomicAdd(totals + img, (uint32_t)tot);
}

__device__ __forceinline__ uint32_t jenc_wave_scan(uint32_t v, int lane)                  // inclusive
{
#pragma unroll
    for (int d = 1; d < 64; d <<= 1) {
        const uint32_t u = __shfl_up(v, d);
        if (lane >= d) v += u;
    }
    return v;
}

// grid (chunks, images), 1024 threads.  A workgroup owns the scan positions [chunk * blockIdx.x, chunk * (blockIdx.x + 1)) of its image:
// it sums the counts before them, scans its own into the image's block table (table[b] .. table[b + 1] are block b's entries, relative to
// the image's first entry; blocks + 1 words) and compacts its blocks: a wave per block, a lane per coefficient, the entry's place from
// the ballot of the non-zero lanes.  The images' entries follow each other: image i starts at the sum of the totals before it.
__global__ __launch_bounds__(JENC_PACK_THREADS) void k_jpegenc_pack(const int16_t* __restrict__ dense, const uint32_t* __restrict__ cnt,
                                                                    const uint32_t* __restrict__ totals, uint32_t* table,
                                                                    uint32_t* __restrict__ entries, int nscan, int chunk)
{
    __shared__ uint32_t red[JENC_PACK_THREADS / 64];
    const int img = blockIdx.y, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, s0 = blockIdx.x * chunk, s1 = min(s0 + chunk, nscan);
    const uint32_t* c = cnt + (size_t)img * nscan;
    uint32_t* tab = table + (size_t)img * (nscan + 1);
    size_t base = 0;
    for (int j = 0; j < img; ++j) base += totals[j];
    uint32_t acc = 0;
    for (int i = tid; i < s0; i += JENC_PACK_THREADS) acc += c[i];
    acc = jenc_wave_scan(acc, lane);
    if (lane == 63) red[wave] = acc;
    __syncthreads();
    uint32_t run = 0;
    for (int k = 0; k < JENC_PACK_THREADS / 64; ++k) run += red[k];
    __syncthreads();
    for (int t0 = s0; t0 < s1; t0 += JENC_PACK_THREADS) {
        const int i = t0 + tid;
        const uint32_t v = i < s1 ? c[i] : 0u, incl = jenc_wave_scan(v, lane);
        if (lane == 63) red[wave] = incl;
        __syncthreads();
        uint32_t before = 0, tile = 0;
        for (int k = 0; k < JENC_PACK_THREADS / 64; ++k) { before += k < wave ? red[k] : 0u; tile += red[k]; }
        if (i < s1) tab[i] = run + before + incl - v;
        run += tile;
        __syncthreads();
    }
    if (s1 == nscan && tid == 0) tab[nscan] = run;
    __syncthreads();                                             // the table words of this chunk are read back below by their own workgroup (`table` is not __restrict__)
    uint32_t* ent = entries + base;
    const uint32_t room = totals[img];                           // what the host sized the image's entries by
    for (int s = s0 + wave; s < s1; s += JENC_PACK_THREADS / 64) {
        if (c[s] == 0u) continue;
        const int v = dense[((size_t)img * nscan + s) * 64 + lane];
        const unsigned long long nz = __ballot(v != 0);
        const uint32_t at = tab[s] + __popcll(nz & ((1ull << lane) - 1ull));
        if (v != 0 && at < room) ent[at] = (uint32_t)lane << 16 | (uint32_t)(uint16_t)v;
    }
}

// ---- device: the entropy stage (docs/JPEG.md section 13) -------------------------------------------------------------------
#define JENC_HLEN_THREADS 256
#define JENC_HLEN_BLOCKS 16             // scan positions per workgroup of k_jpegenc_hlen: four per wave
#define JENC_HW_THREADS 1024
#define JENC_HW_TILE 2048               // k_jpegenc_hwrite's chunks, as k_jpegenc_pack's: ceil(positions / 2048) of them, 16 at the most
#define JENC_HW_CHUNKS 16
#define JENC_HW_WORDS 56                // 31 bits of offset + 1658 bits of block end in word 52; a code's third word may be two further
#define JENC_STUFF_THREADS 256
#define JENC_STUFF_TILE 2048            // bytes per step of a workgroup of k_jpegenc_ffcount / k_jpegenc_stuff: eight per thread
#define JENC_STUFF_CHUNKS 64            // chunks per image at the most (whole tiles each)
#define JENC_HUFF_WORDS (2 * 256 + 2 * 12)

struct JEncHuffDev { uint32_t w[JENC_HUFF_WORDS]; };              // code << 8 | length: AC luma [0, 256), AC chroma [256, 512), DC luma, DC chroma (12 each)
struct JEncGrid { int hm, vm, mcux, nscan, bw, bh; };             // bw, bh: the real luma blocks

// Words of an image's unstuffed stream: whole 8-byte units, so that every image starts 8-byte aligned and the bytes behind its last one are zero
__device__ __host__ __forceinline__ size_t jenc_image_words(unsigned long long bits) { return (size_t)((bits + 63) >> 6) * 2; }
// Bytes of an image's stuffed scan in the stuffed stream (16-byte aligned starts)
__device__ __host__ __forceinline__ size_t jenc_image_room(unsigned long long bits, uint32_t ff) { return (((size_t)((bits + 7) >> 3) + ff) + 15) & ~(size_t)15; }

// Scan position s: is it a real block; t its table (0 luma, 1 chroma); prev the scan position of the nearest earlier REAL block of its component
// (-1: it is the first).  Chroma has no dummies (ceil(ceil(W / hm) / 8) == ceil(W / (8 hm))); of an MCU's hm x vm luma blocks the left
// rw x rh are real, rw = min(hm, bw - mx hm), rh = min(vm, bh - my vm), both at least 1.
__device__ __forceinline__ bool jenc_real(const JEncGrid& g, int s, int& t, int& prev)
{
    const int nl = g.hm * g.vm, bpm = nl + 2, mcu = s / bpm, j = s - mcu * bpm;
    prev = -1;
    if (j >= nl) { t = 1; if (mcu) prev = s - bpm; return true; }
    t = 0;
    const int my = mcu / g.mcux, mx = mcu - my * g.mcux, jy = j / g.hm, jx = j - jy * g.hm;
    const int rw = min(g.hm, g.bw - mx * g.hm), rh = min(g.vm, g.bh - my * g.vm);
    if (jx >= rw || jy >= rh) return false;
    if (jx > 0) prev = s - 1;
    else if (jy > 0) prev = mcu * bpm + (jy - 1) * g.hm + rw - 1;
    else if (mcu > 0) {                                          // the last real block of the MCU before
        const int pm = mcu - 1, pmy = pm / g.mcux, pmx = pm - pmy * g.mcux;
        prev = pm * bpm + (min(g.vm, g.bh - pmy * g.vm) - 1) * g.hm + min(g.hm, g.bw - pmx * g.hm) - 1;
    }
    return true;
}

// The bits lane `lane` contributes to its block: lane 0 the DC difference v, lane k a non-zero AC coefficient v at zig-zag k with the ZRLs of
// the zero run in front of it (nz: the lanes 1 .. 63 with a non-zero value), lane 63 with a zero the EOB.  len <= 3 * 11 + 16 + 10 = 59.
// A category beyond baseline cannot reach this point (section 7, and the host check of the test entry); it is clamped to stay inside the tables.
__device__ __forceinline__ void jenc_lane_code(const uint32_t* hac, const uint32_t* hdc, int lane, int v, unsigned long long nz, uint64_t& bits, int& len)
{
    bits = 0;
    len = 0;
    const int a = v < 0 ? -v : v, mag = v < 0 ? v - 1 : v;
    int s = 32 - __clz(a);
    if (lane == 0) {
        s = min(s, 11);
        const uint32_t e = hdc[s];
        bits = ((uint64_t)(e >> 8) << s) | ((uint32_t)mag & ((1u << s) - 1u));
        len = (int)(e & 0xffu) + s;
    } else if (v != 0) {
        s = min(s, 10);
        const unsigned long long below = nz & ((1ull << lane) - 1ull);
        const int run = lane - 1 - (below ? 63 - __clzll(below) : 0);
        const uint32_t z = hac[0xF0], e = hac[(run & 15) << 4 | s];
        for (int i = 0; i < (run >> 4); ++i) { bits = bits << (z & 0xffu) | (z >> 8); len += (int)(z & 0xffu); }
        const int el = (int)(e & 0xffu) + s;
        bits = bits << el | (uint64_t)(e >> 8) << s | ((uint32_t)mag & ((1u << s) - 1u));
        len += el;
    } else if (lane == 63) {
        const uint32_t e = hac[0];
        bits = e >> 8;
        len = (int)(e & 0xffu);
    }
}

// The block at scan position s of the image whose dense blocks start at d, by one wave: every lane's code; returns the block's bit length.
// A dummy position (never written by k_jpegenc_fdct, never read here) is DC difference 0 and EOB.
__device__ __forceinline__ uint32_t jenc_wave_block(const int16_t* __restrict__ d, const JEncGrid& g, const uint32_t* tab, int s, int lane, uint64_t& bits,
                                                    int& len)
{
    int t, prev, v = 0;
    if (jenc_real(g, s, t, prev)) {
        v = d[(size_t)s * 64 + lane];
        if (lane == 0 && prev >= 0) v -= d[(size_t)prev * 64];
    }
    const unsigned long long nz = __ballot(lane > 0 && v != 0);
    jenc_lane_code(tab + t * 256, tab + 512 + t * 12, lane, v, nz, bits, len);
    uint32_t total = (uint32_t)len;
#pragma unroll
    for (int m = 1; m < 64; m <<= 1) total += __shfl_xor(total, m);
    return total;
}

// grid (ceil(scan positions / 16), images), 256 threads: a wave per block, four blocks per wave.  lens[image][position] = the block's bits;
// bits[image] += them (an integer sum: the same whatever order the atomics land in).
__global__ __launch_bounds__(JENC_HLEN_THREADS) void k_jpegenc_hlen(const int16_t* __restrict__ dense, const JEncGrid g, uint32_t* __restrict__ lens,
                                                                    unsigned long long* __restrict__ bits, const JEncHuffDev T)
{
    __shared__ uint32_t tab[JENC_HUFF_WORDS];
    for (int i = threadIdx.x; i < JENC_HUFF_WORDS; i += JENC_HLEN_THREADS) tab[i] = T.w[i];
    __syncthreads();
    const int img = blockIdx.y, lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int16_t* d = dense + (size_t)img * g.nscan * 64;
    unsigned long long sum = 0;
    for (int b = 0; b < JENC_HLEN_BLOCKS / 4; ++b) {
        const int s = blockIdx.x * JENC_HLEN_BLOCKS + wave * (JENC_HLEN_BLOCKS / 4) + b;
        if (s >= g.nscan) break;                                 // (the same in every lane of the wave)
        uint64_t cb;
        int cl;
        const uint32_t L = jenc_wave_block(d, g, tab, s, lane, cb, cl);
        if (lane == 0) lens[(size_t)img * g.nscan + s] = L;
        sum += L;
    }
    if (lane == 0 && sum) atomicAdd(bits + img, sum);
}

__device__ __forceinline__ void jenc_wave_sync()                 // orders one wave's LDS accesses among its lanes (the hardware serves them in order)
{
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
    __builtin_amdgcn_wave_barrier();
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
}

// grid (chunks, images), 1024 threads.  A workgroup owns the scan positions [chunk * blockIdx.x, chunk * (blockIdx.x + 1)) of its image: it sums the
// lengths before them (64 bits: 3.1 M positions x 1658 bits pass 2^32), scans its own 1024 at a time into LDS and writes its blocks: a wave per
// block, a lane per code, the block's bits merged in the wave's LDS words and every non-zero word ORed into the image's zeroed, big-endian
// stream (atomicOr: the first and the last word are shared with the neighbours; OR does not care in which order they arrive).  The images'
// streams follow each other, jenc_image_words(bits[j]) each.  The workgroup of the last chunk pads the last byte with 1-bits.
__global__ __launch_bounds__(JENC_HW_THREADS) void k_jpegenc_hwrite(const int16_t* __restrict__ dense, const uint32_t* __restrict__ lens,
                                                                    const unsigned long long* __restrict__ bits, uint32_t* ustream, const JEncGrid g, int chunk,
                                                                    const JEncHuffDev T)
{
    __shared__ uint32_t tab[JENC_HUFF_WORDS];
    __shared__ uint32_t red[JENC_HW_THREADS / 64];
    __shared__ unsigned long long tpos[JENC_HW_THREADS];
    __shared__ uint32_t wbuf[JENC_HW_THREADS / 64][JENC_HW_WORDS];
    const int img = blockIdx.y, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, nscan = g.nscan, s0 = blockIdx.x * chunk, s1 = min(s0 + chunk, nscan);
    for (int i = tid; i < JENC_HUFF_WORDS; i += JENC_HW_THREADS) tab[i] = T.w[i];
    const int16_t* d = dense + (size_t)img * nscan * 64;
    const uint32_t* l = lens + (size_t)img * nscan;
    size_t base = 0;
    for (int j = 0; j < img; ++j) base += jenc_image_words(bits[j]);
    const unsigned long long total = bits[img];
    const size_t room = jenc_image_words(total);                 // what the host sized the image's words by
    uint32_t* out = ustream + base;
    uint32_t acc = 0;                                            // at most 3072 lengths per thread, 64 threads per wave: below 2^32
    for (int i = tid; i < s0; i += JENC_HW_THREADS) acc += l[i];
#pragma unroll
    for (int m = 1; m < 64; m <<= 1) acc += __shfl_xor(acc, m);
    if (lane == 0) red[wave] = acc;
    __syncthreads();
    unsigned long long run = 0;
    for (int k = 0; k < JENC_HW_THREADS / 64; ++k) run += red[k];
    __syncthreads();
    for (int t0 = s0; t0 < s1; t0 += JENC_HW_THREADS) {
        const int i = t0 + tid;
        const uint32_t v = i < s1 ? l[i] : 0u, incl = jenc_wave_scan(v, lane);
        if (lane == 63) red[wave] = incl;
        __syncthreads();
        uint32_t before = 0, tile = 0;
        for (int k = 0; k < JENC_HW_THREADS / 64; ++k) { before += k < wave ? red[k] : 0u; tile += red[k]; }
        tpos[tid] = run + before + incl - v;
        run += tile;
        __syncthreads();
        for (int b = 0; b < 64; ++b) {
            const int s = t0 + wave * 64 + b;
            if (s >= s1) break;                                  // (the same in every lane of the wave; no workgroup barrier inside)
            const unsigned long long pos = tpos[wave * 64 + b];
            uint64_t cb;
            int cl;
            (void)jenc_wave_block(d, g, tab, s, lane, cb, cl);
            const uint32_t r = (uint32_t)(pos & 31u) + jenc_wave_scan((uint32_t)cl, lane) - (uint32_t)cl;     // the code's first bit, from the word of `pos`
            if (lane < JENC_HW_WORDS) wbuf[wave][lane] = 0u;
            jenc_wave_sync();
            if (cl) {
                const uint64_t x = cb << (64 - cl);              // top-aligned; the 96-bit window that starts at word r / 32 holds x << (32 - r % 32)
                const uint32_t w0 = r >> 5, sh = r & 31u;
                const uint32_t a0 = (uint32_t)(x >> (32 + sh)), a1 = (uint32_t)(x >> sh), a2 = (uint32_t)((x << (32 - sh)) & 0xffffffffull);
                if (a0) atomicOr(&wbuf[wave][w0], a0);
                if (a1) atomicOr(&wbuf[wave][w0 + 1], a1);
                if (a2) atomicOr(&wbuf[wave][w0 + 2], a2);
            }
            jenc_wave_sync();
            if (lane < JENC_HW_WORDS) {
                const uint32_t w = wbuf[wave][lane];
                const size_t at = (size_t)(pos >> 5) + lane;
                if (w && at < room) atomicOr(out + at, __builtin_bswap32(w));
            }
            jenc_wave_sync();
        }
        __syncthreads();
    }
    if (s1 == nscan && tid == 0 && (total & 7u)) {
        const uint32_t pad = 8u - (uint32_t)(total & 7u), sh = (uint32_t)(total & 31u);
        atomicOr(out + (size_t)(total >> 5), __builtin_bswap32(((1u << pad) - 1u) << (32u - sh - pad)));
    }
}

__device__ __forceinline__ uint32_t jenc_ff_bytes(uint32_t w)
{
    return (uint32_t)((w & 0xffu) == 0xffu) + (uint32_t)((w & 0xff00u) == 0xff00u) + (uint32_t)((w & 0xff0000u) == 0xff0000u) + (uint32_t)(w >= 0xff000000u);
}

// grid (chunks, images), 256 threads.  A workgroup counts the FF bytes in the unstuffed bytes [chunk * blockIdx.x, chunk * (blockIdx.x + 1)) of
// its image (chunk: whole tiles of 2048 bytes): ffc[image][chunk], and fft[image] += it.  The bytes behind an image's last one are zero.
__global__ __launch_bounds__(JENC_STUFF_THREADS) void k_jpegenc_ffcount(const uint32_t* __restrict__ ustream, const unsigned long long* __restrict__ bits,
                                                                        uint32_t* __restrict__ ffc, uint32_t* __restrict__ fft, uint32_t chunk)
{
    __shared__ uint32_t red[JENC_STUFF_THREADS / 64];
    const int img = blockIdx.y, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    size_t base = 0;
    for (int j = 0; j < img; ++j) base += jenc_image_words(bits[j]);
    const uint32_t nbytes = (uint32_t)((bits[img] + 7) >> 3);
    const unsigned long long b0 = (unsigned long long)blockIdx.x * chunk, b1 = b0 + chunk < nbytes ? b0 + chunk : nbytes;
    const uint8_t* src = (const uint8_t*)(ustream + base);
    uint32_t c = 0;
    for (unsigned long long o = b0 + (unsigned long long)tid * 8; o < b1; o += JENC_STUFF_TILE) {
        const uint2 w = *(const uint2*)(src + o);
        c += jenc_ff_bytes(w.x) + jenc_ff_bytes(w.y);
    }
#pragma unroll
    for (int m = 1; m < 64; m <<= 1) c += __shfl_xor(c, m);
    if (lane == 0) red[wave] = c;
    __syncthreads();
    if (tid == 0) {
        c = 0;
        for (int k = 0; k < JENC_STUFF_THREADS / 64; ++k) c += red[k];
        ffc[img * JENC_STUFF_CHUNKS + blockIdx.x] = c;
        if (c) atomicAdd(fft + img, c);
    }
}

// The same grid.  Byte i of the image goes to i + (the FF bytes before i), a 00 behind every FF: the counts of the chunks before, then a scan of
// the threads' own counts per tile.  The images' stuffed scans follow each other, jenc_image_room(bits[j], fft[j]) bytes each.
__global__ __launch_bounds__(JENC_STUFF_THREADS) void k_jpegenc_stuff(const uint32_t* __restrict__ ustream, const unsigned long long* __restrict__ bits,
                                                                      const uint32_t* __restrict__ ffc, const uint32_t* __restrict__ fft,
                                                                      uint8_t* __restrict__ stuffed, uint32_t chunk)
{
    __shared__ uint32_t red[JENC_STUFF_THREADS / 64];
    const int img = blockIdx.y, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    size_t base = 0, sbase = 0;
    for (int j = 0; j < img; ++j) { base += jenc_image_words(bits[j]); sbase += jenc_image_room(bits[j], fft[j]); }
    const uint32_t nbytes = (uint32_t)((bits[img] + 7) >> 3);
    const unsigned long long room = (unsigned long long)nbytes + fft[img];          // what the host sized the image's bytes by
    const unsigned long long b0 = (unsigned long long)blockIdx.x * chunk, b1 = b0 + chunk < nbytes ? b0 + chunk : nbytes;
    const uint8_t* src = (const uint8_t*)(ustream + base);
    uint8_t* dst = stuffed + sbase;
    unsigned long long pre = 0;
    for (int k = 0; k < (int)blockIdx.x; ++k) pre += ffc[img * JENC_STUFF_CHUNKS + k];
    for (unsigned long long t0 = b0; t0 < b1; t0 += JENC_STUFF_TILE) {
        const unsigned long long o = t0 + (unsigned long long)tid * 8;
        uint2 w = make_uint2(0u, 0u);
        if (o < b1) w = *(const uint2*)(src + o);
        const uint32_t c = jenc_ff_bytes(w.x) + jenc_ff_bytes(w.y), incl = jenc_wave_scan(c, lane);
        if (lane == 63) red[wave] = incl;
        __syncthreads();
        uint32_t before = 0, tile = 0;
        for (int k = 0; k < JENC_STUFF_THREADS / 64; ++k) { before += k < wave ? red[k] : 0u; tile += red[k]; }
        unsigned long long at = o + pre + before + incl - c;
#pragma unroll
        for (int k = 0; k < 8; ++k) {
            const uint32_t v = ((k < 4 ? w.x : w.y) >> (8 * (k & 3))) & 0xffu;
            if (o + k < b1 && at < room) dst[at++] = (uint8_t)v;
            if (o + k < b1 && v == 0xffu && at < room) dst[at++] = 0;
        }
        pre += tile;
        __syncthreads();
    }
}

// ---- host: the batch call --------------------------------------------------------------------------------------------------
struct SSJpegEnc {
    struct Slot {
        SsBuf<SS_DEVICE> dense;                                 // device only: every block's 64 values
        SsBuf<SS_DEVICE> cnt;                                   // device only: every block's count
        SsBuf<SS_DEVICE> totals;                                // [64] entries per image
        SsBuf<SS_PINNED> h_totals;
        SsBuf<SS_DEVICE> dev;                                   // the stream: every image's block table, then every image's entries
        SsBuf<SS_PINNED> host;                                  // its pinned host mirror (cacheable: the host threads read it)
        SsEvent ev;
    } slot[2];
    int next = 0;
    struct DSlot {                                              // ss_jpeg_encode_batch_device's own two slots (section 13)
        SsBuf<SS_DEVICE> dense;
        SsBuf<SS_DEVICE> cnt;                                   // k_jpegenc_fdct's counts (written, not used on this path)
        SsBuf<SS_DEVICE> lens;                                  // every block's bit length
        SsBuf<SS_DEVICE> small;                                 // bits [64] (64-bit), totals [64], fft [64], ffc [64][64]
        SsBuf<SS_PINNED> h_small;                               // bits [64] (64-bit), fft [64]
        SsBuf<SS_DEVICE> ustream;                               // the unstuffed streams, zeroed by every call
        SsBuf<SS_DEVICE> stuffed;                               // the stuffed scans
        SsBuf<SS_PINNED> host;                                  // their pinned mirror
        SsEvent ev;
    } dslot[2];
    int dnext = 0;
};

void ss_jpeg_enc_free(SSJpegEnc* j) { delete j; }

// The arguments have been checked (ss_api.hip).  Returns an SS_* code, the message in err.
int ss_jpeg_encode_impl(SSJpegEnc** state, hipStream_t stream, const void* d_in, long long in_frame_stride, int n, int height, int width, int rgb,
                        int quality, int h_samp, int v_samp, int threads, unsigned char* const* out, size_t* out_size, std::string& err)
{
    try {
        if (!*state) *state = new SSJpegEnc();
        SSJpegEnc& S = **state;
        const JEncShape shape(width, height, h_samp, v_samp);
        const int nscan = shape.nscan;
        JEncParams P;
        jenc_quant(quality, P.q);
        for (int t = 0; t < 2; ++t)
            for (int k = 0; k < 64; ++k) P.recip[t][k] = (uint32_t)((1ull << 32) / ((uint32_t)P.q[t][k] << 3)) + 1u;
        for (int k = 0; k < 64; ++k) P.zz[kZigzag[k]] = (uint8_t)k;
        SSJpegEnc::Slot& st = S.slot[S.next];
        const char* const who = "ss_jpeg_encode_batch: ";
        SS_HIPCHK(who, st.ev.ensure());
        SS_HIPCHK(who, st.totals.reserve(64 * sizeof(uint32_t), SS_EXACT));
        SS_HIPCHK(who, st.h_totals.reserve(64 * sizeof(uint32_t), SS_EXACT));
        SS_HIPCHK(who, st.dense.reserve((size_t)n * nscan * 64 * sizeof(int16_t), SS_QUARTER));
        SS_HIPCHK(who, st.cnt.reserve((size_t)n * nscan * sizeof(uint32_t), SS_QUARTER));
        int16_t* dense = st.dense.as<int16_t>();
        uint32_t *cnt = st.cnt.as<uint32_t>(), *totals = st.totals.as<uint32_t>(), *h_totals = st.h_totals.as<uint32_t>();
        // ---- 1. transform; the entry totals decide the size of everything that follows ----
        SS_HIPCHK(who, hipMemsetAsync(totals, 0, n * sizeof(uint32_t), stream));
        hipLaunchKernelGGL(k_jpegenc_fdct, dim3((nscan + 31) / 32, n), dim3(256), 0, stream, (const uint8_t*)d_in, in_frame_stride, height, width, rgb, h_samp,
                           v_samp, shape.mcux, nscan, dense, cnt, totals, P);
        SS_HIPCHK(who, hipGetLastError());
        SS_HIPCHK(who, hipMemcpyAsync(h_totals, totals, n * sizeof(uint32_t), hipMemcpyDeviceToHost, stream));
        SS_HIPCHK(who, hipEventRecord(st.ev, stream));
        SS_HIPCHK(who, hipEventSynchronize(st.ev));
        size_t entries = 0;
        std::vector<size_t> ent_at(n);
        for (int i = 0; i < n; ++i) { ent_at[i] = entries; entries += h_totals[i]; }
        const size_t tab_words = (size_t)n * (nscan + 1), bytes = (tab_words + entries) * 4;
        SS_HIPCHK(who, st.dev.reserve(bytes, SS_QUARTER));
        SS_HIPCHK(who, st.host.reserve(bytes, SS_QUARTER));
        uint32_t* dev = st.dev.as<uint32_t>();
        uint32_t* base = st.host.as<uint32_t>();
        // ---- 2. scan + compaction, ONE copy of exactly the used size ----
        const int chunks = nscan < 16 * 2048 ? (nscan + 2047) / 2048 : 16, chunk = (nscan + chunks - 1) / chunks;
        hipLaunchKernelGGL(k_jpegenc_pack, dim3(chunks, n), dim3(JENC_PACK_THREADS), 0, stream, dense, cnt, totals, dev, dev + tab_words, nscan, chunk);
        SS_HIPCHK(who, hipGetLastError());
        SS_HIPCHK(who, hipMemcpyAsync(base, dev, bytes, hipMemcpyDeviceToHost, stream));
        SS_HIPCHK(who, hipEventRecord(st.ev, stream));
        SS_HIPCHK(who, hipEventSynchronize(st.ev));
        S.next ^= 1;
        // ---- 3. the entropy stage, whole images per thread ----
        std::vector<char> bad(n, 0);
        auto encode = [&](int t, int nt) {
            for (int i = t; i < n; i += nt) {
                const uint32_t* tab = base + (size_t)i * (nscan + 1);
                const uint32_t* ent = base + tab_words + ent_at[i];
                auto block = [tab, ent](int s, int, int, int, uint32_t*, const uint32_t*& e) { e = ent + tab[s]; return (int)(tab[s + 1] - tab[s]); };
                if (!jenc_file(shape, P.q, block, out[i], &out_size[i])) bad[i] = 1;
            }
        };
        if (!run_threads(threads < n ? threads : n, encode)) { err = "ss_jpeg_encode_batch: host encoding failed"; return SS_ERR_INVALID; }
        for (int i = 0; i < n; ++i)
            if (bad[i]) { err = "ss_jpeg_encode_batch: image " + std::to_string(i) + ": a coefficient beyond the baseline categories"; return SS_ERR_INVALID; }
        return SS_OK;
    } catch (...) {
        err = "ss_jpeg_encode_batch: out of memory";
        return SS_ERR_INVALID;
    }
}

// ---- host: the batch call with the entropy stage on the device (docs/JPEG.md section 13) -------------------------------------
static const JEncHuffDev kEncDev = [] {
    JEncHuffDev d;
    for (int t = 0; t < 2; ++t) {
        for (int s = 0; s < 256; ++s) d.w[t * 256 + s] = (uint32_t)kEnc.ac[t].code[s] << 8 | kEnc.ac[t].len[s];
        for (int s = 0; s < 12; ++s) d.w[512 + t * 12 + s] = (uint32_t)kEnc.dc[t].code[s] << 8 | kEnc.dc[t].len[s];
    }
    return d;
}();

// (`who` in what follows: the entry's name with its ": ")
static int jenc_dslot(SSJpegEnc::DSlot& st, const char* who, size_t blocks, std::string& err)
{
    SS_HIPCHK(who, st.ev.ensure());
    SS_HIPCHK(who, st.small.reserve((256 + 64 * JENC_STUFF_CHUNKS) * sizeof(uint32_t), SS_EXACT));
    SS_HIPCHK(who, st.h_small.reserve(192 * sizeof(uint32_t), SS_EXACT));
    SS_HIPCHK(who, st.dense.reserve(blocks * 64 * sizeof(int16_t), SS_QUARTER));
    SS_HIPCHK(who, st.lens.reserve(blocks * sizeof(uint32_t), SS_QUARTER));
    return SS_OK;
}

// Steps 1 .. 6 of section 13 on the n images whose dense blocks are in st.dense.  Three waits on the slot's event: the bit totals size the
// unstuffed stream, the FF totals size the stuffed one, its pinned mirror and the copy, and the copy has to arrive.
static int jenc_entropy_device(SSJpegEnc::DSlot& st, hipStream_t stream, const char* who, int n, const JEncShape& shape, const uint16_t (&q)[2][64], int threads,
                               unsigned char* const* out, size_t* out_size, std::string& err)
{
    const int nscan = shape.nscan;
    const JEncGrid g{shape.hm, shape.vm, shape.mcux, nscan, shape.bw[0], shape.bh[0]};
    unsigned long long* d_bits = st.small.as<unsigned long long>();
    uint32_t *d_fft = st.small.as<uint32_t>() + 192, *d_ffc = st.small.as<uint32_t>() + 256;
    const unsigned long long* h_bits = st.h_small.as<unsigned long long>();
    uint32_t* h_fft = st.h_small.as<uint32_t>() + 128;
    const int16_t* dense = st.dense.as<int16_t>();
    uint32_t* lens = st.lens.as<uint32_t>();
    // ---- 1. every block's bit length; the images' bit totals decide the size of the unstuffed stream ----
    SS_HIPCHK(who, hipMemsetAsync(d_bits, 0, n * sizeof(unsigned long long), stream));
    hipLaunchKernelGGL(k_jpegenc_hlen, dim3((nscan + JENC_HLEN_BLOCKS - 1) / JENC_HLEN_BLOCKS, n), dim3(JENC_HLEN_THREADS), 0, stream, dense, g, lens, d_bits, kEncDev);
    SS_HIPCHK(who, hipGetLastError());
    SS_HIPCHK(who, hipMemcpyAsync(st.h_small.as(), d_bits, n * sizeof(unsigned long long), hipMemcpyDeviceToHost, stream));
    SS_HIPCHK(who, hipEventRecord(st.ev, stream));
    SS_HIPCHK(who, hipEventSynchronize(st.ev));
    size_t words = 0, most = 0;
    for (int i = 0; i < n; ++i) {
        words += jenc_image_words(h_bits[i]);
        const size_t b = (size_t)((h_bits[i] + 7) >> 3);
        if (b > most) most = b;
    }
    SS_HIPCHK(who, st.ustream.reserve(words * 4, SS_QUARTER));
    uint32_t* ustream = st.ustream.as<uint32_t>();
    // ---- 2. scan + write into the zeroed stream, the FF bytes counted; their totals decide the size of everything that follows ----
    SS_HIPCHK(who, hipMemsetAsync(ustream, 0, words * 4, stream));
    SS_HIPCHK(who, hipMemsetAsync(d_fft, 0, n * sizeof(uint32_t), stream));
    const int chunks = nscan < JENC_HW_CHUNKS * JENC_HW_TILE ? (nscan + JENC_HW_TILE - 1) / JENC_HW_TILE : JENC_HW_CHUNKS, chunk = (nscan + chunks - 1) / chunks;
    hipLaunchKernelGGL(k_jpegenc_hwrite, dim3(chunks, n), dim3(JENC_HW_THREADS), 0, stream, dense, lens, d_bits, ustream, g, chunk, kEncDev);
    SS_HIPCHK(who, hipGetLastError());
    const size_t tiles = (most + JENC_STUFF_TILE - 1) / JENC_STUFF_TILE, per = (tiles + JENC_STUFF_CHUNKS - 1) / JENC_STUFF_CHUNKS;
    const uint32_t bchunk = (uint32_t)(per * JENC_STUFF_TILE);
    const int bchunks = (int)((most + bchunk - 1) / bchunk);
    hipLaunchKernelGGL(k_jpegenc_ffcount, dim3(bchunks, n), dim3(JENC_STUFF_THREADS), 0, stream, ustream, d_bits, d_ffc, d_fft, bchunk);
    SS_HIPCHK(who, hipGetLastError());
    SS_HIPCHK(who, hipMemcpyAsync(h_fft, d_fft, n * sizeof(uint32_t), hipMemcpyDeviceToHost, stream));
    SS_HIPCHK(who, hipEventRecord(st.ev, stream));
    SS_HIPCHK(who, hipEventSynchronize(st.ev));
    size_t bytes = 0;
    std::vector<size_t> at(n);
    for (int i = 0; i < n; ++i) { at[i] = bytes; bytes += jenc_image_room(h_bits[i], h_fft[i]); }
    SS_HIPCHK(who, st.stuffed.reserve(bytes, SS_QUARTER));
    SS_HIPCHK(who, st.host.reserve(bytes, SS_QUARTER));
    uint8_t* stuffed = st.stuffed.as<uint8_t>();
    uint8_t* base = st.host.as<uint8_t>();
    // ---- 3. stuffing, ONE copy of exactly the used size ----
    hipLaunchKernelGGL(k_jpegenc_stuff, dim3(bchunks, n), dim3(JENC_STUFF_THREADS), 0, stream, ustream, d_bits, d_ffc, d_fft, stuffed, bchunk);
    SS_HIPCHK(who, hipGetLastError());
    SS_HIPCHK(who, hipMemcpyAsync(base, stuffed, bytes, hipMemcpyDeviceToHost, stream));
    SS_HIPCHK(who, hipEventRecord(st.ev, stream));
    SS_HIPCHK(who, hipEventSynchronize(st.ev));
    // ---- 4. header, scan, EOI: whole images per thread ----
    auto write = [&](int t, int nt) {
        for (int i = t; i < n; i += nt) {
            const size_t len = (size_t)((h_bits[i] + 7) >> 3) + h_fft[i];
            uint8_t* p = jenc_header(out[i], shape, q);
            memcpy(p, base + at[i], len);
            p += len;
            *p++ = 0xFF; *p++ = 0xD9;
            out_size[i] = (size_t)(p - out[i]);
        }
    };
    if (!run_threads(threads < n ? threads : n, write)) { err = std::string(who) + "host copy failed"; return SS_ERR_INVALID; }
    return SS_OK;
}

// The arguments have been checked (ss_api.hip).  Returns an SS_* code, the message in err.
int ss_jpeg_encode_device_impl(SSJpegEnc** state, hipStream_t stream, const void* d_in, long long in_frame_stride, int n, int height, int width, int rgb,
                               int quality, int h_samp, int v_samp, int threads, unsigned char* const* out, size_t* out_size, std::string& err)
{
    const char* who = "ss_jpeg_encode_batch_device: ";
    try {
        if (!*state) *state = new SSJpegEnc();
        SSJpegEnc& S = **state;
        const JEncShape shape(width, height, h_samp, v_samp);
        const int nscan = shape.nscan;
        JEncParams P;
        jenc_quant(quality, P.q);
        for (int t = 0; t < 2; ++t)
            for (int k = 0; k < 64; ++k) P.recip[t][k] = (uint32_t)((1ull << 32) / ((uint32_t)P.q[t][k] << 3)) + 1u;
        for (int k = 0; k < 64; ++k) P.zz[kZigzag[k]] = (uint8_t)k;
        SSJpegEnc::DSlot& st = S.dslot[S.dnext];
        if (const int rc = jenc_dslot(st, who, (size_t)n * nscan, err)) return rc;
        SS_HIPCHK(who, st.cnt.reserve((size_t)n * nscan * sizeof(uint32_t), SS_QUARTER));
        uint32_t* totals = st.small.as<uint32_t>() + 128;        // (k_jpegenc_fdct's entry totals: written, not used on this path)
        SS_HIPCHK(who, hipMemsetAsync(totals, 0, n * sizeof(uint32_t), stream));
        hipLaunchKernelGGL(k_jpegenc_fdct, dim3((nscan + 31) / 32, n), dim3(256), 0, stream, (const uint8_t*)d_in, in_frame_stride, height, width, rgb, h_samp,
                           v_samp, shape.mcux, nscan, st.dense.as<int16_t>(), st.cnt.as<uint32_t>(), totals, P);
        SS_HIPCHK(who, hipGetLastError());
        S.dnext ^= 1;
        return jenc_entropy_device(st, stream, who, n, shape, P.q, threads, out, out_size, err);
    } catch (...) {
        err = std::string(who) + "out of memory";
        return SS_ERR_INVALID;
    }
}

// The entropy stage alone on one image's coefficients (ss_jpeg_coefficients' layout), for tests.  Categories beyond baseline are refused here,
// before anything is launched, with the host writer's message.
int ss_jpeg_entropy_encode_device_impl(SSJpegEnc** state, hipStream_t stream, const short* coef, int quality, int width, int height, int h_samp, int v_samp,
                                       unsigned char* out, size_t* out_size, std::string& err)
{
    const char* who = "ss_jpeg_entropy_encode_device: ";
    try {
        if (!*state) *state = new SSJpegEnc();
        SSJpegEnc& S = **state;
        const JEncShape shape(width, height, h_samp, v_samp);
        uint16_t q[2][64];
        jenc_quant(quality, q);
        std::vector<int16_t> dense((size_t)shape.nscan * 64, 0);  // scan order, zig-zag order: what k_jpegenc_fdct leaves
        const size_t ybl = (size_t)shape.mcux * shape.hm * shape.mcuy * shape.vm, cbl = (size_t)shape.mcux * shape.mcuy;
        int pred[3] = {0, 0, 0}, s = 0;
        for (int my = 0; my < shape.mcuy; ++my)
            for (int mx = 0; mx < shape.mcux; ++mx)
                for (int j = 0; j < shape.bpm; ++j, ++s) {
                    const int comp = j < shape.hm * shape.vm ? 0 : 1 + j - shape.hm * shape.vm, t = comp ? 1 : 0;
                    const int by = comp ? my : my * shape.vm + j / shape.hm, bx = comp ? mx : mx * shape.hm + j % shape.hm;
                    if (by >= shape.bh[t] || bx >= shape.bw[t]) continue;
                    const short* c = coef + (comp == 0 ? ((size_t)by * shape.mcux * shape.hm + bx) : ybl + (comp - 1) * cbl + (size_t)by * shape.mcux + bx) * 64;
                    int16_t* o = dense.data() + (size_t)s * 64;
                    bool ok = jenc_category(c[0] - pred[comp]) <= 11;
                    pred[comp] = c[0];
                    for (int k = 0; k < 64; ++k) { o[k] = c[kZigzag[k]]; if (k && jenc_category(o[k]) > 10) ok = false; }
                    if (!ok) { err = std::string(who) + "a coefficient beyond the baseline categories (DC difference 11 bits, AC 10 bits)"; return SS_ERR_INVALID; }
                }
        SSJpegEnc::DSlot& st = S.dslot[S.dnext];
        if (const int rc = jenc_dslot(st, who, (size_t)shape.nscan, err)) return rc;
        SS_HIPCHK(who, hipMemcpyAsync(st.dense.as(), dense.data(), dense.size() * sizeof(int16_t), hipMemcpyHostToDevice, stream));
        S.dnext ^= 1;
        return jenc_entropy_device(st, stream, who, 1, shape, q, 1, &out, out_size, err);      // (its first wait is behind the upload: `dense` outlives it)
    } catch (...) {
        err = std::string(who) + "out of memory";
        return SS_ERR_INVALID;
    }
}
