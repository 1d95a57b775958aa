// Transport 3 of a device group (group.hip): the processes of a group meet in a POSIX shared-memory segment named after the group id.
// Plain host code -- no HIP: the two copies between a device and a ring slot are callables of the caller -- so that the protocol
// (attaching to a possibly stale segment, the chunk rings, the all-gather area with its two buffers and sequence numbers) runs as a program
// of its own under the sanitizers, ranks as threads (tests/cpp/group_link_host.cpp).  Every wait has a deadline: a peer that died is an
// error, not a hang.  A call reports {code, text, broken}; the caller owns the group's error text and its broken flag.
#pragma once
#include "../../include/mi355x_groth16.h"
#include <atomic>
#include <chrono>
#include <cstdio>
#include <cstring>
#include <string>
#include <thread>
#include <vector>
#include <fcntl.h>
#include <sys/mman.h>
#include <sys/stat.h>
#include <unistd.h>

static constexpr uint32_t SHM_MAGIC = 0x6d693335u, SHM_MAX_WORLD = 64, SHM_AG_MAX = 1024;
struct alignas(64) ShmRing { std::atomic<uint64_t> head; char pad0[56]; std::atomic<uint64_t> tail; char pad1[56]; };   // chunks produced (by the source) / consumed (by the destination)
struct alignas(64) ShmAg { std::atomic<uint64_t> seq; char pad[56]; unsigned char data[2][SHM_AG_MAX]; };              // collective k writes data[k & 1], then seq = k
struct ShmHeader {
    std::atomic<uint32_t> magic;      // set by rank 0 when the header is initialised
    uint32_t world, nslot;
    uint64_t chunk;                   // bytes per ring slot
    std::atomic<uint32_t> attached;   // ranks that have mapped the segment
    std::atomic<uint32_t> poisoned;   // a rank hit a transport error: everyone waiting gives up at once
    std::atomic<uint64_t> beat;       // rank 0 counts here while it waits for the others to attach: a segment whose count stands still has no creator any more
    ShmAg ag[SHM_MAX_WORLD];
    ShmRing ring[SHM_MAX_WORLD * SHM_MAX_WORLD];   // ring[src * world + dst]
};
static constexpr size_t SHM_HEADER_BYTES = (sizeof(ShmHeader) + 4095) & ~(size_t)4095;   // the rings' slots start here

struct Xfer { int src, dst; const void *sp; void *dp; size_t bytes; };   // global ranks; a pointer is meaningful in its owner's process only
struct LinkStatus {
    int32_t code = MI_OK;
    std::string text;       // empty where a callable of the caller failed: its text is the caller's already
    bool broken = false;    // the rings / the all-gather area are in an unknown state: nothing collective can follow
};
struct Deadline {
    std::chrono::steady_clock::time_point t;
    explicit Deadline(int ms) : t(std::chrono::steady_clock::now() + std::chrono::milliseconds(ms)) {}
    bool passed() const { return std::chrono::steady_clock::now() > t; }
};
static inline void shm_pause(unsigned &spins) {
    if (++spins < 200) std::this_thread::yield();
    else std::this_thread::sleep_for(std::chrono::microseconds(50));
}
static inline std::string shm_name_of(const uint8_t id[128]) {
    uint64_t h = 1469598103934665603ull;   // FNV-1a over the 128 id bytes
    for (int i = 0; i < 128; i++) { h ^= id[i]; h *= 1099511628211ull; }
    char buf[64];
    snprintf(buf, sizeof buf, "/mi355x_grp_%016llx", (unsigned long long)h);
    return buf;
}

struct ShmLink {
    ShmHeader *h = nullptr;
    unsigned char *data = nullptr;    // ring r, slot k: data + ((size_t)r * nslot + k) * chunk
    size_t map_bytes = 0;
    uint64_t ag_seq = 0;              // collectives of the all-gather area this rank has entered (all ranks in lockstep)
    int world = 0, rank = 0, timeout_ms = 60000;

    size_t ring_bytes() const { return (size_t)h->nslot * h->chunk; }
    bool poisoned() const { return h && h->poisoned.load(std::memory_order_acquire) != 0; }
    void poison() { if (h) h->poisoned.store(1, std::memory_order_release); }
    LinkStatus fail(const char *msg) { poison(); return {MI_EHIP, msg, true}; }

    // Rank 0 creates and initialises the segment, the others map it as soon as it shows its magic; once every rank is attached rank 0
    // unlinks the name, so that nothing outlives the processes whatever way they end.
    LinkStatus attach(const std::string &name, int rank_, int world_, int timeout_ms_, uint64_t chunk, uint32_t nslot) {
        world = world_; rank = rank_; timeout_ms = timeout_ms_;
        const int W = world;
        const size_t hdr = SHM_HEADER_BYTES;
        if (W > (int)SHM_MAX_WORLD) return {MI_EINVAL, "group: the host-staged transport serves at most 64 ranks", false};
        const Deadline dl(timeout_ms);
        if (rank == 0) {
            (void)shm_unlink(name.c_str());   // a leftover of a run that died before everyone had attached
            const int fd = shm_open(name.c_str(), O_CREAT | O_EXCL | O_RDWR, 0600);
            if (fd < 0) return {MI_EHIP, "group: shm_open (create) failed", false};
            map_bytes = hdr + (size_t)W * W * nslot * chunk;   // tmpfs allocates a page when it is first touched: rings nobody uses cost nothing
            if (ftruncate(fd, (off_t)map_bytes) != 0) { close(fd); (void)shm_unlink(name.c_str()); return {MI_ENOMEM, "group: ftruncate of the shared segment failed", false}; }
            void *m = mmap(nullptr, map_bytes, PROT_READ | PROT_WRITE, MAP_SHARED, fd, 0);
            close(fd);
            if (m == MAP_FAILED) { (void)shm_unlink(name.c_str()); return {MI_ENOMEM, "group: mmap of the shared segment failed", false}; }
            h = (ShmHeader *)m;
            data = (unsigned char *)m + hdr;
            // (a fresh tmpfs file reads as zeros: rings, sequence numbers and flags start at 0)
            h->world = (uint32_t)W; h->nslot = nslot; h->chunk = chunk;
            h->magic.store(SHM_MAGIC, std::memory_order_release);
        } else {
            // The name may still point at the segment of an EARLIER group with the same id (a run that died before rank 0 unlinked it, or rank
            // 0 of this run has not replaced it yet): its magic and shape look right.  A segment is this group's only if, once its magic shows,
            // the NAME still leads to the same file -- rank 0 unlinks a leftover before it creates, and unlinks its own only after every rank
            // (this one included) has attached.  Anything else is unmapped and the name is tried again until the deadline.
            unsigned spins = 0;
            for (;;) {
                if (dl.passed()) return {MI_EHIP, "group: rank 0 never created (or initialised) the shared segment (timeout)", false};
                const int fd = shm_open(name.c_str(), O_RDWR, 0600);
                struct stat sb;
                if (fd < 0 || fstat(fd, &sb) != 0 || (size_t)sb.st_size < hdr) { if (fd >= 0) close(fd); shm_pause(spins); continue; }   // not there / not sized yet
                const size_t bytes = (size_t)sb.st_size;
                void *m = mmap(nullptr, bytes, PROT_READ | PROT_WRITE, MAP_SHARED, fd, 0);
                close(fd);
                if (m == MAP_FAILED) return {MI_ENOMEM, "group: mmap of the shared segment failed", false};
                ShmHeader *hh = (ShmHeader *)m;
                bool mine = false;
                while (!dl.passed()) {
                    if (hh->magic.load(std::memory_order_acquire) == SHM_MAGIC) {
                        const int fd2 = shm_open(name.c_str(), O_RDWR, 0600);
                        struct stat sb2;
                        mine = fd2 >= 0 && fstat(fd2, &sb2) == 0 && sb2.st_ino == sb.st_ino && sb2.st_dev == sb.st_dev;
                        if (fd2 >= 0) close(fd2);
                        if (mine) {   // ... and its creator is alive: rank 0 counts h->beat while it waits for us (a leftover's stands still)
                            const uint64_t b0 = hh->beat.load(std::memory_order_acquire);
                            const Deadline alive(timeout_ms < 1000 ? timeout_ms : 1000);
                            while (hh->beat.load(std::memory_order_acquire) == b0 && !alive.passed()) shm_pause(spins);
                            mine = hh->beat.load(std::memory_order_acquire) != b0;
                        }
                        break;
                    }
                    shm_pause(spins);
                }
                if (mine && (int)hh->world == W && hdr + (size_t)W * W * hh->nslot * hh->chunk <= bytes) { h = hh; data = (unsigned char *)m + hdr; map_bytes = bytes; break; }
                (void)munmap(m, bytes);
                if (mine) return {MI_EINVAL, "group: the shared segment belongs to a group of another shape", false};
                shm_pause(spins);   // a leftover: try the name again
            }
        }
        h->attached.fetch_add(1, std::memory_order_acq_rel);
        unsigned spins = 0;
        while ((int)h->attached.load(std::memory_order_acquire) < W) {
            if (dl.passed()) { if (rank == 0) (void)shm_unlink(name.c_str()); return {MI_EHIP, "group: not every rank attached to the shared segment (timeout)", false}; }
            if (rank == 0) h->beat.fetch_add(1, std::memory_order_release);
            shm_pause(spins);
        }
        if (rank == 0) (void)shm_unlink(name.c_str());
        return {};
    }
    void detach() {
        if (h) (void)munmap((void *)h, map_bytes);
        h = nullptr; data = nullptr;
    }
    // all-gather of `bytes` (<= SHM_AG_MAX) per rank through the segment's all-gather area
    LinkStatus allgather(const void *local, size_t bytes, void *all) {
        if (bytes > SHM_AG_MAX) return {MI_EINVAL, "group: all-gather payload too large", false};
        const uint64_t k = ++ag_seq;
        ShmAg &mine = h->ag[rank];
        std::memcpy(mine.data[k & 1], local, bytes);
        mine.seq.store(k, std::memory_order_release);
        const Deadline dl(timeout_ms);
        for (int r = 0; r < world; r++) {
            unsigned spins = 0;
            // (a rank may be one collective ahead -- it then wrote the OTHER buffer -- never two: collective k + 1 completes only once
            //  every rank has entered it, i.e. has finished reading k)
            while (h->ag[r].seq.load(std::memory_order_acquire) < k) {
                if (poisoned()) return {MI_EHIP, "group: another rank reported a transport failure", true};
                if (dl.passed()) return fail("group: a rank did not reach the all-gather (timeout; did its process end?)");
                shm_pause(spins);
            }
            std::memcpy((char *)all + (size_t)r * bytes, h->ag[r].data[k & 1], bytes);
        }
        return {};
    }
    // Every transfer this process takes part in advances chunk by chunk through ring[src][dst] -- the source copies a chunk
    // device -> slot and publishes it (head), the destination copies slot -> device and releases it (tail).  A process both sends and
    // receives in one batch and the rings are finite, so the two directions are interleaved in ONE progress loop (two ranks that each
    // first sent everything would wait for each other's free slots forever).  Transfers of one (src, dst) pair complete in list order
    // (the ring is a FIFO and both sides build the same list).
    // copy_out(slot, source, bytes) / copy_in(destination, slot, bytes): the caller's copies, complete on return; MI_OK or the call's status.
    template <class CopyOut, class CopyIn>
    LinkStatus run_xfers(const std::vector<Xfer> &list, CopyOut copy_out, CopyIn copy_in) {
        const int W = world, me = rank;
        const size_t chunk = (size_t)h->chunk, nslot = h->nslot;
        struct St { size_t sent = 0, rcvd = 0; };
        std::vector<St> st(list.size());
        Deadline dl(timeout_ms);   // the time this rank may WAIT for its peers without any chunk moving (renewed by every chunk)
        unsigned spins = 0;
        for (;;) {
            bool all_done = true, progress = false;
            std::vector<char> pair_send_busy((size_t)W * W, 0), pair_recv_busy((size_t)W * W, 0);
            for (size_t k = 0; k < list.size(); k++) {
                const Xfer &x = list[k];
                if (!x.bytes) continue;
                const size_t pr = (size_t)x.src * W + x.dst;
                ShmRing &ring = h->ring[pr];
                unsigned char *slots = data + pr * nslot * chunk;
                if (x.src == me && st[k].sent < x.bytes) {
                    all_done = false;
                    if (!pair_send_busy[pr]) {
                        pair_send_busy[pr] = 1;   // later transfers of this pair wait for this one
                        uint64_t head = ring.head.load(std::memory_order_relaxed);
                        while (st[k].sent < x.bytes && head - ring.tail.load(std::memory_order_acquire) < nslot) {
                            const size_t nb = x.bytes - st[k].sent < chunk ? x.bytes - st[k].sent : chunk;
                            if (const int32_t rc = copy_out(slots + (head % nslot) * chunk, (const char *)x.sp + st[k].sent, nb)) return {rc, "", false};
                            st[k].sent += nb;
                            ring.head.store(++head, std::memory_order_release);
                            progress = true;
                        }
                    }
                }
                if (x.dst == me && st[k].rcvd < x.bytes) {
                    all_done = false;
                    if (!pair_recv_busy[pr]) {
                        pair_recv_busy[pr] = 1;
                        uint64_t tail = ring.tail.load(std::memory_order_relaxed);
                        while (st[k].rcvd < x.bytes && tail < ring.head.load(std::memory_order_acquire)) {
                            const size_t nb = x.bytes - st[k].rcvd < chunk ? x.bytes - st[k].rcvd : chunk;
                            if (const int32_t rc = copy_in((char *)x.dp + st[k].rcvd, slots + (tail % nslot) * chunk, nb)) return {rc, "", false};
                            st[k].rcvd += nb;
                            ring.tail.store(++tail, std::memory_order_release);
                            progress = true;
                        }
                    }
                }
            }
            if (all_done) return {};
            if (progress) { spins = 0; dl = Deadline(timeout_ms); continue; }
            if (poisoned()) return {MI_EHIP, "group: another rank reported a transport failure", true};
            if (dl.passed()) return fail("group: a peer did not take part in the exchange (timeout; did its process end?)");
            shm_pause(spins);
        }
    }
};
