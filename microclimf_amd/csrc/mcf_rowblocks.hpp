// mcf_rowblocks.hpp — host only: what the entries that cut one raster into row blocks and drive them with one host thread
// per device share (the solver and bioclim `_multi` entries in mcf_api.hip, mcf_precompute_terrain_multi, the snow model
// and the snow run in mcf_snowrun.hip): the device list, the worker pool and its per-block loop, row gather / scatter, the host copies
// an input struct is re-pointed at, the solver inputs' block view.
#pragma once

#include <hip/hip_runtime.h>
#include <stdint.h>
#include <string.h>

#include <atomic>
#include <condition_variable>
#include <deque>
#include <exception>
#include <mutex>
#include <string>
#include <thread>
#include <vector>

#include "../../include/mcf.h"

namespace mcf {

int api_fail(int code, const std::string& msg);   // mcf_api.hip: sets the calling thread's mcf_last_error()

// R's NA_real_
inline double na_real_host() {
    const uint64_t u = 0x7FF00000000007A2ULL;
    double d;
    memcpy(&d, &u, 8);
    return d;
}

// The devices of a call: with `mu`, its list (n_devices <= 0: every visible device), without it `device` alone.
// devs = nullptr: only the check.
inline int device_list(const mcf_multi* mu, int device, std::vector<int>* devs) {
    int nd = 0;
    if (hipGetDeviceCount(&nd) != hipSuccess || nd <= 0)
        return api_fail(MCF_ERR_NO_DEVICE, "no HIP device available (libmcfhip has no CPU fallback)");
    if (mu && mu->n_devices > 0 && !mu->devices) return api_fail(MCF_ERR_ARG, "n_devices > 0 with a null device list");
    const int n = !mu ? 1 : mu->n_devices > 0 ? mu->n_devices : nd;
    for (int i = 0; i < n; ++i) {
        const int d = !mu ? device : mu->n_devices > 0 ? mu->devices[i] : i;
        if (d < 0 || d >= nd) return api_fail(MCF_ERR_ARG, "device ordinal out of range");
        if (devs) devs->push_back(d);
    }
    return MCF_OK;
}
inline int check_device(int device) { return device_list(nullptr, device, nullptr); }

// the calling thread's current device, put back when this goes out of scope
struct RestoreDevice {
    int device = -1;
    RestoreDevice() { if (hipGetDevice(&device) != hipSuccess) device = -1; }
    ~RestoreDevice() { if (device >= 0) (void)hipSetDevice(device); }
};

struct PhaseBarrier {
    std::mutex m;
    std::condition_variable cv;
    int n, waiting = 0, generation = 0;
    explicit PhaseBarrier(int n_) : n(n_) {}
    void wait() {
        std::unique_lock<std::mutex> lk(m);
        const int g = generation;
        if (++waiting == n) { waiting = 0; ++generation; cv.notify_all(); }
        else cv.wait(lk, [&] { return g != generation; });
    }
};

// what the workers of one run_workers call share
struct WorkerPool {
    explicit WorkerPool(int nt) : bar(nt), rcs((size_t)nt, MCF_OK), errs((size_t)nt) {}
    PhaseBarrier bar;
    std::atomic<bool> failed{false};
    std::vector<int> rcs;              // each worker's first error
    std::vector<std::string> errs;
};

// Worker t of run_workers drives the blocks t, t + nt, ...  Every worker runs every phase, also after a failure (the barrier
// counts heads): a phase body run under guarded() is skipped once any worker has failed, and no exception leaves it —
// std::terminate would take the host R / Python process down, a skipped barrier would hang the others.
struct Worker {
    int t;
    WorkerPool& pool;
    void wait() { pool.bar.wait(); }
    bool failed() const { return pool.failed; }
    void fail(int rc) { record(rc, mcf_last_error()); }
    template <class B>
    void guarded(B&& body) {
        if (pool.failed) return;
        try { body(); }
        catch (const std::exception& e) { record(MCF_ERR_NOMEM, std::string("row-block worker: ") + e.what()); }
    }
    void record(int rc, const std::string& err) {
        if (pool.rcs[(size_t)t] == MCF_OK) { pool.rcs[(size_t)t] = rc; pool.errs[(size_t)t] = err; }
        pool.failed = true;
    }
};

// body(b) for worker w's blocks b = w.t, w.t + nt, ... < nb, under guarded(): the first non-zero return is recorded as the
// worker's failure and ends its loop.  No barrier: the caller places those.
template <class B>
void for_blocks(Worker& w, int nb, int nt, B&& body) {
    w.guarded([&] {
        for (int b = w.t; b < nb && !w.failed(); b += nt)
            if (const int rc = body(b)) { w.fail(rc); break; }
    });
}
// What every block reported in the phase before is combined by worker 0 alone, between two barriers (partial sums added in
// block order: a run is reproducible for a given number of blocks).
template <class B>
void reduce_on_first(Worker& w, B&& body) {
    w.wait();
    if (w.t == 0) w.guarded(body);
    w.wait();
}

// fn(Worker&) on nt workers: worker 0 on the calling thread, the others on threads of their own.  Returns the error of the
// lowest-numbered failing worker; the calling thread's current device is put back.
template <class F>
int run_workers(int nt, F&& fn) {
    RestoreDevice restore;
    WorkerPool pool(nt);
    auto work = [&](int t) {
        Worker w{t, pool};
        try { fn(w); }
        catch (const std::exception& e) { w.record(MCF_ERR_NOMEM, std::string("row-block worker: ") + e.what()); }
    };
    std::vector<std::thread> threads;
    for (int t = 1; t < nt; ++t) threads.emplace_back(work, t);
    work(0);
    for (auto& th : threads) th.join();
    for (int t = 0; t < nt; ++t)
        if (pool.rcs[(size_t)t] != MCF_OK) return api_fail(pool.rcs[(size_t)t], pool.errs[(size_t)t]);
    return MCF_OK;
}

// rows r0 .. r0 + nr of a column-major [R, C, layers] array into a dense [nr, C, layers] one ...
template <class T>
void gather_rows(std::vector<T>& dst, const T* src, int64_t R, int64_t C, int64_t r0, int64_t nr, int64_t layers = 1) {
    dst.resize((size_t)(nr * C * layers));
    for (int64_t lc = 0; lc < C * layers; ++lc) memcpy(&dst[(size_t)(nr * lc)], src + r0 + R * lc, (size_t)nr * sizeof(T));
}
// ... and back
template <class T>
void scatter_rows(T* dst, const T* src, int64_t R, int64_t C, int64_t r0, int64_t nr, int64_t layers = 1) {
    for (int64_t lc = 0; lc < C * layers; ++lc) memcpy(dst + r0 + R * lc, src + nr * lc, (size_t)nr * sizeof(T));
}

// Host copies that an input struct is pointed at — a block's own rows of a raster, the selected days of a series — kept for as
// long as the struct is used.
struct HostCopies {
    std::deque<std::vector<double>> f64;
    std::deque<std::vector<int32_t>> i32;
    std::vector<double>& fresh(const double*) { f64.emplace_back(); return f64.back(); }
    std::vector<int32_t>& fresh(const int32_t*) { i32.emplace_back(); return i32.back(); }
    template <class T>
    const T* rows(const T* src, int64_t R, int64_t C, int64_t r0, int64_t nr, int64_t layers) {     // gather_rows
        std::vector<T>& v = fresh(src);
        gather_rows(v, src, R, C, r0, nr, layers);
        return v.data();
    }
    // the rows of the selected days out of a whole-series hourly table: day d of `src` becomes day sub_of_day[d] (>= 0) of nsub
    template <class T>
    const T* days(const T* src, const int32_t* sub_of_day, int ndays, int nsub) {
        std::vector<T>& v = fresh(src);
        v.resize((size_t)nsub * 24);
        for (int d = 0; d < ndays; ++d)
            if (sub_of_day[d] >= 0) memcpy(&v[(size_t)sub_of_day[d] * 24], src + (size_t)d * 24, 24 * sizeof(T));
        return v.data();
    }
};

// The block view of the solver's inputs: rows r0 .. r0 + nr of the caller's arrays, read in place through the row pitch.  The
// array-forcing series are offset only for array_forcing == 1 (coarse forcing keeps its own grid).
inline mcf_grid_inputs narrow_rows(const mcf_grid_inputs& in, int64_t r0, int64_t nr, int64_t pitch) {
    mcf_grid_inputs sub = in;
    sub.rows = nr;
    sub.row_pitch = pitch;
    auto off = [&](const double*& q) { if (q) q += r0; };
    off(sub.vegp.hgt); off(sub.vegp.pai); off(sub.vegp.x); off(sub.vegp.gsmax); off(sub.vegp.leafr); off(sub.vegp.leaft);
    off(sub.vegp.clump); off(sub.vegp.leafd); off(sub.vegp.paia); off(sub.vegp.leafden);
    off(sub.soilc.Smin); off(sub.soilc.Smax); off(sub.soilc.gref); off(sub.soilc.soilb); off(sub.soilc.Psie);
    off(sub.soilc.Vq); off(sub.soilc.Vm); off(sub.soilc.Mc); off(sub.soilc.rho); off(sub.soilc.slope);
    off(sub.soilc.aspect); off(sub.soilc.twi); off(sub.soilc.svfa); off(sub.soilc.wsa); off(sub.soilc.hor);
    off(sub.lats); off(sub.lons); off(sub.coarse_rowpos); off(sub.fine_dtm);
    if (in.array_forcing == 1) {
        off(sub.clim.tc); off(sub.clim.es); off(sub.clim.ea); off(sub.clim.tdew); off(sub.clim.pk); off(sub.clim.swdown);
        off(sub.clim.difrad); off(sub.clim.lwdown); off(sub.clim.windspeed);
        off(sub.pointm.soilm); off(sub.pointm.G); off(sub.pointm.umu); off(sub.pointm.kp); off(sub.pointm.muGp);
        off(sub.pointm.dtrp); off(sub.pointm.Tg); off(sub.pointm.Tbp);
    }
    return sub;
}

}  // namespace mcf
