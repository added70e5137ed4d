// The two host helpers the tracker families' states are built on (csrc/ss_host.h), as a program of its own for the host compiler and
// its sanitizers: ss_carve_plan, the offset plan of one buffer's tables, and ss_gather_rows, the list-order read-back.  No device call
// is made.  Prints what it checked; any difference is a message on stderr and exit status 1.
#include <cstdio>
#include <cstdlib>
#include <numeric>
#include <vector>
#include "../include/strongsort_hip.h"
#include "../strongsort_yolo_amd/csrc/ss_host.h"

static int failures = 0;
#define EXPECT(cond, ...) do { if (!(cond)) { std::fprintf(stderr, __VA_ARGS__); std::fputc('\n', stderr); ++failures; } } while (0)

// every offset on a 256-byte boundary, the ranges disjoint and in registration order, the total covering the last table
static void plan(const std::vector<size_t>& bytes)
{
    std::vector<size_t> off(bytes.size(), ~(size_t)0);
    const size_t total = ss_carve_plan(bytes.data(), bytes.size(), off.data());
    size_t end = 0;
    for (size_t i = 0; i < bytes.size(); ++i) {
        EXPECT(off[i] % 256 == 0, "table %zu of %zu: offset %zu is not a multiple of 256", i, bytes.size(), off[i]);
        EXPECT(off[i] >= end, "table %zu of %zu: offset %zu starts inside the table before it (ends at %zu)", i, bytes.size(), off[i], end);
        end = off[i] + bytes[i];
    }
    EXPECT(total >= end, "total %zu does not cover the last table (ends at %zu)", total, end);
    EXPECT(total < end + 256, "total %zu wastes a whole boundary past %zu", total, end);
}

// n slots in a permuted order out of a [SS_MAX_TRACKS][width] table, against a plain double loop; a NULL destination writes nothing
template <class T>
static void gather(int width, int n, unsigned seed)
{
    const int rows = SS_MAX_TRACKS;
    std::vector<T> src((size_t)rows * width);
    for (size_t i = 0; i < src.size(); ++i) src[i] = (T)(i * 2654435761u + seed);
    std::vector<int> slots(rows);
    std::iota(slots.begin(), slots.end(), 0);
    for (int i = rows - 1; i > 0; --i) {                              // a fixed shuffle: every slot once, none in its place's order
        seed = seed * 1664525u + 1013904223u;
        std::swap(slots[i], slots[seed % (unsigned)(i + 1)]);
    }
    const T mark = (T)77;
    std::vector<T> got((size_t)n * width + 1, mark), want((size_t)n * width + 1, mark);      // one element past the end: stays untouched
    for (int i = 0; i < n; ++i)
        for (int k = 0; k < width; ++k) want[(size_t)i * width + k] = src[(size_t)slots[i] * width + k];
    ss_gather_rows(slots.data(), n, src.data(), width, got.data());
    EXPECT(got == want, "gather of %d slots, width %d, element size %zu differs from the double loop", n, width, sizeof(T));
    ss_gather_rows(slots.data(), n, src.data(), width, (T*)nullptr);
}

int main()
{
    const std::vector<std::vector<size_t>> plans = {
        {4}, {1, 255, 256, 257, 4096}, {0, 0, 8, 0}, {}, {2 * 256 * 4, 2 * 256 * 49 * 8, 0, 2 * 256 * 128 * 8, 3},
    };
    for (const auto& p : plans) plan(p);
    int gathers = 0;
    for (int width : {1, 2, 8, 49})
        for (int n : {0, 1, SS_MAX_TRACKS}) {
            gather<int>(width, n, 1u + gathers); gather<unsigned>(width, n, 2u + gathers);
            gather<float>(width, n, 3u + gathers); gather<double>(width, n, 4u + gathers);
            gathers += 4;
        }
    std::printf("plans %zu gathers %d failures %d\n", plans.size(), gathers, failures);
    return failures ? 1 : 0;
}
