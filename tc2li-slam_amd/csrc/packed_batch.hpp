// The way of a problem batch through the device, as every batched entry goes it: the caller's per-problem tables are concatenated into
// one pinned buffer [inputs | state with initial values | outputs], each table on a 256-byte boundary; parts one and two go up in one
// copy, the kernels run, parts two and three come down in one copy, the stream is waited on and the entry scatters the results into the
// problems' arrays.  Here: the layout (Packer), the buffers kept between calls (PackedBuffers, PackedSpace), the copies and the wait (PackedTransfer),
// the per-problem validation, the row limit of the 32-bit kernels, and what the entries with capacities share.  An entry writes its
// sizes, its tables, its batch structure and its scatter back.
#pragma once
#include <algorithm>
#include <cstring>

#include "common.hpp"

namespace tc2li {

// Tables packed into one buffer, each on a 256-byte boundary: take() hands out the places, put() / get() copy `count` entries of `width`
// bytes to / from entry `start` of the table at o, once base is the buffer.  take<T>(count) gives the place of `count` entries of T as a
// Table<T>: the pointers and copies made from it need no type or width again.
template <class T> struct Table { size_t o = 0; };
struct Packer {
    uint8_t* base = nullptr;
    size_t off = 0;
    size_t take(size_t bytes) { const size_t o = off; off = align256(off + bytes); return o; }
    template <class T> Table<T> take(size_t count) { return Table<T>{take(count * sizeof(T))}; }
    void put(size_t o, size_t start, const void* src, size_t count, size_t width) const {
        if (count) memcpy(base + o + start * width, src, count * width);
    }
    void get(void* dst, size_t o, size_t start, size_t count, size_t width) const {
        if (count) memcpy(dst, base + o + start * width, count * width);
    }
    template <class T> void put(Table<T> t, size_t start, const void* src, size_t count) const { put(t.o, start, src, count, sizeof(T)); }
    template <class T> void get(void* dst, Table<T> t, size_t start, size_t count) const { get(dst, t.o, start, count, sizeof(T)); }
};

// The buffers of an entry, kept between calls: a work space of one host thread (thread_local) holds them as they are.  PackedSpace adds
// the mutex of a process-wide one, held for the length of a call; every such entry has its own through shutdown_owned<PackedSpace, tag>,
// so none waits for another.
struct PackedBuffers {
    DevBuf<uint8_t> io, work;
    PinnedBuf<uint8_t> h_io;
};
struct PackedSpace : PackedBuffers {
    std::mutex mu;
};
enum PackedSpaceTag { kSpaceKeyframeCulling, kSpaceMapPointCulling, kSpaceConnections, kSpaceCovisibles, kSpaceStereoPoints, kSpaceMlpnp, kSpaceInertialWindow, kSpaceInertialTerm,
                      kSpaceScaledRotation, kSpaceGbaCorrection, kSpaceInertialInit, kSpaceLocalMap, kSpaceNeighbors, kSpaceProcessKeyframe };

// One call's transfer.  The entry take()s its inputs from io, calls state_begins() and takes the tables that go up and come back (an
// entry without such tables skips this), calls outputs_begin() and takes what does not go up with the block -- its outputs, or tables it
// uploads later by themselves; it takes its work tables from work.  Then (a process-wide space: under its lock): ensure(), the tables
// put into io, upload(), zero_work() where the kernels expect zeros, the launch, and download_and_wait() or the entry's own downloads.
struct PackedTransfer {
    Packer io, work;
    size_t up_bytes = 0, down_from = ~(size_t)0;
    uint8_t *d_io = nullptr, *d_work = nullptr;

    void state_begins() { down_from = io.off; }
    void outputs_begin() { up_bytes = io.off; down_from = std::min(down_from, io.off); }
    // the work buffer is never empty: an entry may zero or point into it whatever its sizes are
    hipError_t ensure(PackedBuffers& S) {
        hipError_t e = S.io.ensure(io.off);
        if (e == hipSuccess) e = S.work.ensure(std::max(work.off, (size_t)256));
        if (e == hipSuccess) e = S.h_io.ensure(io.off);
        io.base = S.h_io.p;   // put / get work on the host copy
        d_io = S.io.p; d_work = S.work.p;
        return e;
    }
    hipError_t upload(hipStream_t st) const { return hipMemcpyAsync(d_io, io.base, up_bytes, hipMemcpyHostToDevice, st); }
    // the first `bytes` of the work buffer
    hipError_t zero_work(size_t bytes, hipStream_t st) const { return hipMemsetAsync(d_work, 0, std::max(bytes, (size_t)256), st); }
    hipError_t download(size_t from, size_t to, hipStream_t st) const {
        return hipMemcpyAsync(io.base + from, d_io + from, to - from, hipMemcpyDeviceToHost, st);
    }
    hipError_t download_and_wait(hipStream_t st) const {
        const hipError_t e = download(down_from, io.off, st);
        return e == hipSuccess ? stream_wait_blocking(st) : e;
    }
    // the table at o: on the device, in the device's work buffer, in the pinned copy
    template <class T> T* dev(size_t o) const { return (T*)(d_io + o); }
    template <class T> T* dev_work(size_t o) const { return (T*)(d_work + o); }
    template <class T> T* host(size_t o) const { return (T*)(io.base + o); }
    template <class T> T* dev(Table<T> t) const { return (T*)(d_io + t.o); }
    template <class T> T* dev_work(Table<T> t) const { return (T*)(d_work + t.o); }
    template <class T> T* host(Table<T> t) const { return (T*)(io.base + t.o); }
    // entries start .. start + count of one table up again: what the host rewrote after a wait
    template <class T> hipError_t upload(Table<T> t, size_t start, size_t count, hipStream_t st) const {
        return hipMemcpyAsync(dev(t) + start, host(t) + start, count * sizeof(T), hipMemcpyHostToDevice, st);
    }
};

// ---- validation ------------------------------------------------------------------------------------------------------------------------
// check(i, &what) for every item on the tracking pool: 0, or the error's code with what set.  The first failure in item order is the
// one reported, as "<entry>: <noun> <i>: <what>".
template <class Check>
int validate_each(const char* entry, const char* noun, int n, Check check) {
    std::vector<const char*> what(n, "");
    std::vector<int> code(n, 0);
    tracking_pool().parallel_for(n, [&](int i) { code[i] = check(i, &what[i]); });
    for (int i = 0; i < n; ++i)
        if (code[i]) {
            set_error("%s: %s %d: %s", entry, noun, i, what[i]);
            return code[i];
        }
    return 0;
}
// a check from what_of(i): "" or what is wrong, which is TC2LI_ERR_INVALID
template <class WhatOf>
auto invalid_if(WhatOf what_of) {
    return [what_of](int i, const char** what) { *what = what_of(i); return (*what)[0] ? TC2LI_ERR_INVALID : 0; };
}

// the kernels index the concatenated tables with 32 bits
constexpr size_t kMaxRows = 0x7fffff00u;
inline int too_many_rows(const char* entry, int p) {
    set_error("%s: the batch up to problem %d has more than 2^31 rows in one table; split it", entry, p);
    return TC2LI_ERR_INVALID;
}

// ---- capacities ------------------------------------------------------------------------------------------------------------------------
// A host entry whose lists may not fit: one(p, write) sizes problem p, writes its lists when asked to, and returns whether they fit.
// Sizes first: on TC2LI_ERR_CAPACITY -- capacity_error(p) sets the error and returns the code -- no list of any problem is written.
template <class One, class CapacityError>
int size_then_write(int n_problems, One one, CapacityError capacity_error) {
    std::vector<uint8_t> ok(n_problems, 1);
    tracking_pool().parallel_for(n_problems, [&](int p) { ok[p] = one(p, false); });
    for (int p = 0; p < n_problems; ++p)
        if (!ok[p]) return capacity_error(p);
    tracking_pool().parallel_for(n_problems, [&](int p) { one(p, true); });
    return n_problems;
}

// The downloaded counts (n_counts per problem) into the problems' arrays; fits(problem, counts).  Returns the first problem short of
// room, or -1.
template <class Problem, class Fits>
int copy_counts(const Problem* problems, int n_problems, const int32_t* counts, int n_counts, Fits fits) {
    int short_of_room = -1;
    for (int p = 0; p < n_problems; ++p, counts += n_counts) {
        memcpy(problems[p].counts, counts, (size_t)n_counts * 4);
        if (short_of_room < 0 && !fits(problems[p], counts)) short_of_room = p;
    }
    return short_of_room;
}

}  // namespace tc2li
