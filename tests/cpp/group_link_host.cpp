// Stand-alone host run of the shared-memory link of a device group (gnark-whir_amd/csrc/group_link.h: attaching to a possibly stale
// segment, the chunk rings, the all-gather area, the poison flag and the deadlines): built with -fsanitize=address,undefined by
// `make sanitize-group-link`, run by tests/test_group_link_cpu.py.  Ranks are threads, each with a link object and a mapping of the
// segment of its own; memcpy stands in for the two device copies.  Every buffer is a heap block of exactly its length, so a copy past
// an end is an error the sanitizer reports.  Every group has a fresh random id.  Chunks of 4 KB, 4 slots, worlds 2, 3 and 4 (side by
// side).  Prints "group link host: ok".
#include <atomic>
#include <chrono>
#include <cstdio>
#include <cstring>
#include <functional>
#include <memory>
#include <random>
#include <string>
#include <thread>
#include <vector>
#include "../../gnark-whir_amd/csrc/group_link.h"

namespace {

constexpr uint64_t CHUNK = 4096;
constexpr uint32_t NSLOT = 4;
constexpr size_t RING = CHUNK * NSLOT;
const char *const T_BATCH = "group: a peer did not take part in the exchange (timeout; did its process end?)";
const char *const T_GATHER = "group: a rank did not reach the all-gather (timeout; did its process end?)";
const char *const T_TOLD = "group: another rank reported a transport failure";

std::atomic<int> fails{0};
void expect(bool ok, const std::string &what) {
    if (!ok) { std::printf("FAIL: %s\n", what.c_str()); fails++; }
}
std::string fresh_name() {
    uint8_t id[128];
    std::random_device rd;
    for (uint8_t &b : id) b = (uint8_t)rd();
    return shm_name_of(id);
}
void each_rank(int W, const std::function<void(int)> &fn) {
    std::vector<std::thread> th;
    for (int r = 0; r < W; r++) th.emplace_back(fn, r);
    for (std::thread &t : th) t.join();
}
int32_t plain_copy(void *dst, const void *src, size_t nb) { std::memcpy(dst, src, nb); return MI_OK; }
unsigned char pat(int src, int dst, size_t k, int salt = 0) { return (unsigned char)(17 * src + 101 * dst + 3 * k + (k >> 8) + 29 * salt); }
using Block = std::unique_ptr<unsigned char[]>;
Block block(size_t n) { return Block(new unsigned char[n ? n : 1]); }

struct Group {
    int W;
    std::string name = fresh_name();
    std::vector<ShmLink> link;
    explicit Group(int W_) : W(W_), link((size_t)W_) {}
    void form(const std::string &what) {
        each_rank(W, [&](int r) {
            const LinkStatus s = link[r].attach(name, r, W, 20000, CHUNK, NSLOT);
            expect(s.code == MI_OK && !s.broken, what + ": attach of rank " + std::to_string(r) + ": " + s.text);
        });
    }
    ~Group() { for (ShmLink &l : link) l.detach(); }
};

// every rank sends `bytes` patterned bytes to every rank (itself included) in ONE batch -- both directions at once, the interleaving
// rule of the progress loop -- and checks what it received
void all_to_all(Group &G, size_t bytes, const std::string &what) {
    const int W = G.W;
    each_rank(W, [&](int me) {
        std::vector<Block> snd, rcv;
        for (int o = 0; o < W; o++) {
            snd.push_back(block(bytes)); rcv.push_back(block(bytes));
            for (size_t k = 0; k < bytes; k++) snd[o][k] = pat(me, o, k);
            std::memset(rcv[o].get(), 0, bytes);
        }
        std::vector<Xfer> list;   // the same list on every rank; a pointer is set by its owner only
        for (int s = 0; s < W; s++) for (int d = 0; d < W; d++) list.push_back({s, d, s == me ? snd[d].get() : nullptr, d == me ? rcv[s].get() : nullptr, bytes});
        const LinkStatus st = G.link[me].run_xfers(list, plain_copy, plain_copy);
        expect(st.code == MI_OK && !st.broken, what + ": batch of rank " + std::to_string(me) + ": " + st.text);
        bool same = true;
        for (int s = 0; s < W; s++) for (size_t k = 0; k < bytes; k++) same = same && rcv[s][k] == pat(s, me, k);
        expect(same, what + ": rank " + std::to_string(me) + " received wrong bytes");
    });
}

// two transfers of the pair (0, 1) in one batch, with a zero-byte transfer (null pointers) between them: the ring is a FIFO, so the
// second lands only after the first, and each lands whole in its own block
void same_pair_in_list_order(Group &G, const std::string &what) {
    const size_t n1 = RING + 5000, n2 = 3000;
    Block s1 = block(n1), s2 = block(n2), d1 = block(n1), d2 = block(n2);
    for (size_t k = 0; k < n1; k++) s1[k] = pat(0, 1, k, 1);
    for (size_t k = 0; k < n2; k++) s2[k] = pat(0, 1, k, 2);
    std::memset(d1.get(), 0, n1); std::memset(d2.get(), 0, n2);
    std::vector<int> order;   // rank 1: which block every incoming chunk went to
    each_rank(G.W, [&](int me) {
        const std::vector<Xfer> list = {{0, 1, me == 0 ? s1.get() : nullptr, me == 1 ? d1.get() : nullptr, n1}, {0, 1, nullptr, nullptr, 0},
                                        {0, 1, me == 0 ? s2.get() : nullptr, me == 1 ? d2.get() : nullptr, n2}};
        auto copy_in = [&](void *dst, const void *src, size_t nb) {
            order.push_back((unsigned char *)dst >= d2.get() && (unsigned char *)dst < d2.get() + n2 ? 2 : 1);
            return plain_copy(dst, src, nb);
        };
        const LinkStatus st = G.link[me].run_xfers(list, plain_copy, copy_in);
        expect(st.code == MI_OK && !st.broken, what + ": batch of rank " + std::to_string(me) + ": " + st.text);
    });
    bool sorted = true;
    for (size_t k = 1; k < order.size(); k++) sorted = sorted && order[k - 1] <= order[k];
    expect(sorted && order.size() == (n1 + CHUNK - 1) / CHUNK + 1, what + ": the second transfer of a pair overtook the first");
    bool same = true;
    for (size_t k = 0; k < n1; k++) same = same && d1[k] == pat(0, 1, k, 1);
    for (size_t k = 0; k < n2; k++) same = same && d2[k] == pat(0, 1, k, 2);
    expect(same, what + ": wrong bytes");
}

// 1000 all-gathers in a row, a distinct value per rank and round; the last rank sleeps every few rounds, so that its peers run one
// collective ahead of it and write the OTHER buffer of the area
void many_allgathers(Group &G, const std::string &what) {
    const int W = G.W;
    each_rank(W, [&](int me) {
        std::vector<uint64_t> all(2 * (size_t)W);
        bool same = true, ok = true;
        for (uint64_t round = 0; round < 1000; round++) {
            if (me == W - 1 && round % 7 == 3) std::this_thread::sleep_for(std::chrono::milliseconds(1));
            const uint64_t mine[2] = {round * 1000003u + (uint64_t)me, ~round ^ ((uint64_t)me << 40)};
            const LinkStatus st = G.link[me].allgather(mine, sizeof mine, all.data());
            ok = ok && st.code == MI_OK && !st.broken;
            for (int r = 0; r < W; r++) same = same && all[2 * r] == round * 1000003u + (uint64_t)r && all[2 * r + 1] == (~round ^ ((uint64_t)r << 40));
        }
        expect(ok, what + ": an all-gather of rank " + std::to_string(me) + " failed");
        expect(same, what + ": rank " + std::to_string(me) + " read a value of another round or rank");
    });
}
void allgather_sizes(Group &G, const std::string &what) {
    const int W = G.W;
    each_rank(W, [&](int me) {
        Block mine = block(SHM_AG_MAX + 1), all = block((size_t)W * SHM_AG_MAX);
        for (size_t k = 0; k <= SHM_AG_MAX; k++) mine[k] = pat(me, 0, k, 3);
        LinkStatus st = G.link[me].allgather(mine.get(), SHM_AG_MAX + 1, all.get());
        expect(st.code == MI_EINVAL && !st.broken && st.text == "group: all-gather payload too large", what + ": a payload of SHM_AG_MAX + 1 bytes must be refused");
        st = G.link[me].allgather(mine.get(), SHM_AG_MAX, all.get());
        expect(st.code == MI_OK && !st.broken, what + ": a payload of SHM_AG_MAX bytes: " + st.text);
        bool same = true;
        for (int r = 0; r < W; r++) for (size_t k = 0; k < SHM_AG_MAX; k++) same = same && all[(size_t)r * SHM_AG_MAX + k] == pat(r, 0, k, 3);
        expect(same, what + ": wrong bytes in the largest payload");
    });
}

// The last rank never enters a collective.  With a deadline of 200 ms every other rank returns within 2 s, broken, and the link reads
// poisoned.  The rank whose deadline passes first returns the timeout text and poisons the segment; a rank that sees the flag before its
// own deadline returns "another rank reported a transport failure" (with two ranks there is no such rank).
void absent_rank(int W, bool gather, const std::string &what) {
    Group G(W);
    G.form(what);
    std::vector<LinkStatus> got((size_t)W);
    std::vector<double> seconds((size_t)W, 0);
    each_rank(W, [&](int me) {
        if (me == W - 1) return;
        G.link[me].timeout_ms = 200;
        Block snd = block(100), rcv = block((size_t)W * 100), all = block((size_t)W * 8);
        std::memset(snd.get(), me, 100);
        std::vector<Xfer> list;
        for (int s = 0; s < W; s++) for (int d = 0; d < W; d++) list.push_back({s, d, s == me ? snd.get() : nullptr, d == me ? rcv.get() + (size_t)s * 100 : nullptr, 100});
        const uint64_t mine = (uint64_t)me;
        const auto t0 = std::chrono::steady_clock::now();
        got[me] = gather ? G.link[me].allgather(&mine, 8, all.get()) : G.link[me].run_xfers(list, plain_copy, plain_copy);
        seconds[me] = std::chrono::duration<double>(std::chrono::steady_clock::now() - t0).count();
    });
    int timed_out = 0;
    for (int r = 0; r + 1 < W; r++) {
        const bool timeout_text = got[r].text == (gather ? T_GATHER : T_BATCH);
        timed_out += timeout_text ? 1 : 0;
        expect(got[r].code == MI_EHIP && got[r].broken && (timeout_text || (W > 2 && got[r].text == T_TOLD)), what + ": rank " + std::to_string(r) + " returned: " + got[r].text);
        expect(seconds[r] < 2.0, what + ": rank " + std::to_string(r) + " took " + std::to_string(seconds[r]) + " s");
        expect(G.link[r].poisoned(), what + ": the link of rank " + std::to_string(r) + " does not read poisoned");
    }
    expect(timed_out >= 1, what + ": no rank returned the timeout text");
}

// A segment of an EARLIER group is still under the name: valid magic and shape, nobody counting its heartbeat.  Rank 0 starts after
// the others.  The group forms on rank 0's new segment, moves correct bytes, and nobody has touched the leftover.
void leftover_segment(int W, const std::string &what) {
    Group G(W);
    const size_t bytes = SHM_HEADER_BYTES + (size_t)W * W * NSLOT * CHUNK;
    const int fd = shm_open(G.name.c_str(), O_CREAT | O_EXCL | O_RDWR, 0600);
    void *m = fd >= 0 && ftruncate(fd, (off_t)bytes) == 0 ? mmap(nullptr, bytes, PROT_READ | PROT_WRITE, MAP_SHARED, fd, 0) : MAP_FAILED;
    if (fd >= 0) close(fd);
    expect(m != MAP_FAILED, what + ": the test could not create its leftover segment");
    if (m == MAP_FAILED) { (void)shm_unlink(G.name.c_str()); return; }
    ShmHeader *old = (ShmHeader *)m;
    old->world = (uint32_t)W; old->nslot = NSLOT; old->chunk = CHUNK;
    old->magic.store(SHM_MAGIC, std::memory_order_release);
    each_rank(W, [&](int slot) {
        const int r = (slot + 1) % W;   // rank 0 is started last ...
        if (r == 0) std::this_thread::sleep_for(std::chrono::milliseconds(100));   // ... and late: the others have met the leftover by then
        const LinkStatus s = G.link[r].attach(G.name, r, W, 20000, CHUNK, NSLOT);
        expect(s.code == MI_OK && !s.broken, what + ": attach of rank " + std::to_string(r) + ": " + s.text);
    });
    bool formed = true;
    for (const ShmLink &l : G.link) formed = formed && l.h != nullptr && l.h != old;
    if (formed) all_to_all(G, 5000, what);
    expect(old->attached.load() == 0 && old->ring[1].head.load() == 0 && old->ag[0].seq.load() == 0, what + ": a rank used the leftover segment");
    (void)munmap(m, bytes);
    (void)shm_unlink(G.name.c_str());   // (rank 0 has unlinked the name already, unless the group did not form)
}

void world(int W) {
    const std::string w = "world " + std::to_string(W);
    {
        Group G(W);
        G.form(w);
        // one chunk and its neighbours; exactly the ring and one byte over it; several ring lengths with a ragged tail
        for (size_t bytes : {(size_t)1, (size_t)4095, (size_t)4096, (size_t)4097, RING, RING + 1, 5 * RING + 777}) all_to_all(G, bytes, w + ", all-to-all of " + std::to_string(bytes) + " bytes");
        same_pair_in_list_order(G, w + ", two transfers of one pair");
        many_allgathers(G, w + ", 1000 all-gathers");
        allgather_sizes(G, w + ", all-gather sizes");
        all_to_all(G, 4097, w + ", a batch after the all-gathers");
    }
    absent_rank(W, false, w + ", a rank that never enters a batch");
    absent_rank(W, true, w + ", a rank that never enters an all-gather");
    leftover_segment(W, w + ", a leftover segment under the name");
}

}  // namespace

int main() {
    static_assert(RING == 16384, "the sizes below are one chunk, the ring, and one byte over it");
    std::vector<std::thread> th;
    for (int W : {2, 3, 4}) th.emplace_back(world, W);
    for (std::thread &t : th) t.join();
    if (fails.load()) { std::printf("group link host: %d failure(s)\n", fails.load()); return 1; }
    std::printf("group link host: ok\n");
    return 0;
}
