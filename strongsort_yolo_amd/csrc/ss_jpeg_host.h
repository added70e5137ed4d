// ss_jpeg_host.h — what the host stages of the JPEG decoder (ss_jpeg.hip) and encoder (ss_jpeg_enc.hip) share.
#pragma once
#include <cstdint>
#include <thread>
#include <vector>

static const uint8_t kZigzag[64] = {0, 1, 8, 16, 9, 2, 3, 10, 17, 24, 32, 25, 18, 11, 4, 5, 12, 19, 26, 33, 40, 48, 41, 34, 27, 20, 13, 6, 7, 14, 21, 28,
                                    35, 42, 49, 56, 57, 50, 43, 36, 29, 22, 15, 23, 30, 37, 44, 51, 58, 59, 52, 45, 38, 31, 39, 46, 53, 60, 61, 54, 47, 55, 62, 63};

// ss_upload_batch's rules: threads that cannot be started have their share done by the caller; nothing thrown crosses the C boundary
template <class Work>
static bool run_threads(int T, Work work)
{
    try {
        std::vector<std::thread> pool;
        pool.reserve(T > 1 ? T - 1 : 0);
        int started = 1;
        try {
            for (int t = 1; t < T; ++t) { pool.emplace_back(work, t, T); ++started; }
        } catch (...) {
            for (auto& th : pool) th.join();
            for (int t = started; t < T; ++t) work(t, T);
            pool.clear();
        }
        work(0, T);
        for (auto& th : pool) th.join();
    } catch (...) {
        return false;
    }
    return true;
}
