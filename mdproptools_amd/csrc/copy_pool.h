// copy_pool.h — the helper threads that fill the page-locked ring of mdhip_h2d_any (mdhip_ctx.hip). Standard library
// only, so that tests/native/copy_pool_main.cpp can run it on its own under the thread and address sanitizers.
#pragma once

#include <algorithm>
#include <cstddef>
#include <cstring>

#include <condition_variable>
#include <mutex>
#include <thread>

struct CopyPool {
    static constexpr int N = 4;
    struct Job {
        char *dst = nullptr;
        const char *src = nullptr;
        size_t n = 0;
    };
    std::thread th[N];
    std::mutex mu;
    std::condition_variable cv_go, cv_done;
    Job job[N];
    unsigned long long gen = 0;
    int left = 0;
    bool quit = false;
    CopyPool()
    {
        for (int k = 0; k < N; ++k) th[k] = std::thread([this, k]() { run(k); });
    }
    ~CopyPool()
    {
        {
            std::lock_guard<std::mutex> lk(mu);
            quit = true;
            ++gen;
        }
        cv_go.notify_all();
        for (auto &t : th) t.join();
    }
    void run(int k)
    {
        unsigned long long seen = 0;
        for (;;) {
            Job j;
            {
                std::unique_lock<std::mutex> lk(mu);
                cv_go.wait(lk, [&]() { return gen != seen; });
                seen = gen;
                if (quit) return;
                j = job[k];
            }
            if (j.n) memcpy(j.dst, j.src, j.n);
            {
                std::lock_guard<std::mutex> lk(mu);
                if (--left == 0) cv_done.notify_one();
            }
        }
    }
    // dst[0, n) = src[0, n), split over the helpers; returns when done
    void copy(void *dst, const void *src, size_t n)
    {
        const size_t per = ((n + N - 1) / N + 63) & ~size_t(63);
        {
            std::lock_guard<std::mutex> lk(mu);
            for (int k = 0; k < N; ++k) {
                const size_t o = std::min(n, per * k), e = std::min(n, per * (k + 1));
                job[k] = {static_cast<char *>(dst) + o, static_cast<const char *>(src) + o, e - o};
            }
            left = N;
            ++gen;
        }
        cv_go.notify_all();
        std::unique_lock<std::mutex> lk(mu);
        cv_done.wait(lk, [&]() { return left == 0; });
    }
};
