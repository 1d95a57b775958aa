// Mutation driver for the host-only walk over a proving key's stream in either encoding: mi_pk_stream_inspect (and mi_pk_stream_size
// over what it reports).  Compiled TOGETHER with csrc/keyfile_inspect.hip as plain C++ under -fsanitize=address,undefined
// (gnark-whir_amd/Makefile `sanitize-keyfile`; tests/test_keyfile_cpu.py builds and runs it on the CPU -- sanitizers belong on this
// build only).  Test infrastructure.
//
//   keyfile_fuzz <raw.bin> <compressed.bin> <iterations> <seed>
//
// Both seed files are VALID streams of one key (the driver first checks that each is accepted, in its own encoding, with the same
// counts).  Mutations: every truncation (sampled on long seeds), bit flips, byte writes, 4- and 8-byte big-endian counts overwritten
// with 0, 1, 2^31, 2^32 - 1 and values near the input's own length, random blobs, splices -- also of one encoding's head onto the
// other's tail.  Every mutant is copied into a heap block of exactly its size, so a read past the input is the sanitizer's to find.
// Exit status 0 = no sanitizer report and no broken contract (an accepted stream names sections that lie inside it, one after the other,
// and has the length mi_pk_stream_size computes from its counts).  Prints "accepted refused".
#include "../../include/mi355x_groth16_keyfile.h"
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

typedef std::vector<uint8_t> Bytes;
static uint64_t rng_state = 1;
static uint64_t rnd() { uint64_t z = (rng_state += 0x9e3779b97f4a7c15ull); z = (z ^ (z >> 30)) * 0xbf58476d1ce4e5b9ull; z = (z ^ (z >> 27)) * 0x94d049bb133111ebull; return z ^ (z >> 31); }
static size_t below(size_t n) { return n ? (size_t)(rnd() % n) : 0; }

static Bytes read_file(const char *path) {
    Bytes b;
    FILE *f = fopen(path, "rb");
    if (!f) { fprintf(stderr, "keyfile_fuzz: cannot open %s\n", path); exit(2); }
    uint8_t buf[65536];
    size_t n;
    while ((n = fread(buf, 1, sizeof buf, f)) > 0) b.insert(b.end(), buf, buf + n);
    fclose(f);
    return b;
}
[[noreturn]] static void broken(const char *what) { fprintf(stderr, "keyfile_fuzz: %s\n", what); exit(3); }

static unsigned long n_accept, n_refuse;

// true = accepted; info and encoding as the library left them
static bool run(const Bytes &in, mi_pk_raw_info *info, uint32_t *encoding) {
    uint8_t *exact = (uint8_t *)malloc(in.size() ? in.size() : 1);   // no slack behind the last byte
    if (!in.empty()) memcpy(exact, in.data(), in.size());
    const int32_t rc = mi_pk_stream_inspect(exact, in.size(), info, encoding);
    if (rc != MI_OK) { n_refuse++; free(exact); return false; }
    n_accept++;
    if (*encoding > MI_KEYFILE_COMPRESSED) broken("an accepted stream has no known encoding");
    const uint64_t g1 = *encoding == MI_KEYFILE_COMPRESSED ? 32 : 64, g2 = 2 * g1;
    uint64_t at = 8 + 5 * 32 + 1;
    auto section = [&](uint64_t off, unsigned __int128 bytes, uint64_t gap) {   // gap: the count in front of it
        if (off != at + gap || (unsigned __int128)off + bytes > in.size()) broken("a section is not where the layout puts it, or leaves the input");
        at = off + (uint64_t)bytes;
    };
    section(info->off_alpha1, 3 * g1, 0);
    section(info->off_g1_a, (unsigned __int128)info->n_g1_a * g1, 4); section(info->off_g1_b, (unsigned __int128)info->n_g1_b * g1, 4);
    section(info->off_g1_z, (unsigned __int128)info->n_g1_z * g1, 4); section(info->off_g1_k, (unsigned __int128)info->n_g1_k * g1, 4);
    section(info->off_beta2, 2 * g2, 0);
    section(info->off_g2_b, (unsigned __int128)info->n_g2_b * g2, 4);
    section(info->off_infinity_a, (info->nb_wires + 7) / 8, 3 * 8 + 4); section(info->off_infinity_b, (info->nb_wires + 7) / 8, 4);
    if (info->n_commitment_keys > MI_PK_RAW_MAX_COMMITMENTS) broken("more Pedersen keys than the info has room for");
    mi_pedersen_arrays ped[MI_PK_RAW_MAX_COMMITMENTS];
    for (uint32_t k = 0; k < info->n_commitment_keys; k++) {
        section(info->off_basis[k], (unsigned __int128)info->n_basis[k] * g1, k ? 4 : 8);
        section(info->off_basis_exp_sigma[k], (unsigned __int128)info->n_basis[k] * g1, 4);
        ped[k] = mi_pedersen_arrays{nullptr, nullptr, info->n_basis[k]};
    }
    // the size computed from the counts is the size of the stream
    mi_pk_desc d;
    memset(&d, 0, sizeof d);
    d.nb_wires = info->nb_wires; d.n_g1_a = info->n_g1_a; d.n_g1_b = info->n_g1_b; d.n_g1_z = info->n_g1_z; d.n_g1_k = info->n_g1_k; d.n_g2_b = info->n_g2_b;
    size_t len = 0;
    if (mi_pk_stream_size(&d, ped, info->n_commitment_keys, *encoding, &len) != MI_OK || len != in.size()) broken("mi_pk_stream_size disagrees with an accepted stream");
    // the flag bits of the first point belong to the encoding
    const unsigned flag = exact[info->off_alpha1] >> 6;
    if (*encoding == MI_KEYFILE_RAW ? flag > 1 : flag == 0) broken("the first point's flag bits belong to the other encoding");
    free(exact);
    return true;
}

static Bytes mutate(const Bytes &seed, const Bytes &other) {
    Bytes m = seed;
    switch ((int)below(7)) {
        case 0: m.resize(below(m.size() + 1)); break;
        case 1: for (size_t k = 0, f = 1 + below(4); k < f && !m.empty(); k++) m[below(m.size())] ^= (uint8_t)(1u << below(8)); break;
        case 2: for (size_t k = 0, f = 1 + below(4); k < f && !m.empty(); k++) m[below(m.size())] = (uint8_t)rnd(); break;
        case 3: {   // a 4- or 8-byte big-endian count
            if (m.size() < 9) break;
            const uint64_t vals[] = {0, 1, 0xffffffffull, 0x80000000ull, (uint64_t)m.size(), (uint64_t)m.size() / 32, (uint64_t)m.size() / 64, rnd()};
            const uint64_t v = vals[below(sizeof vals / sizeof vals[0])];
            const int w = below(2) ? 4 : 8;
            const size_t off = below(m.size() - 8);
            for (int k = 0; k < w; k++) m[off + k] = (uint8_t)(v >> (8 * (w - 1 - k)));
            break;
        }
        case 4: m.assign(below(400), 0); for (auto &x : m) x = (uint8_t)rnd(); break;
        case 5: m.resize(below(m.size() + 1)); m.insert(m.end(), other.begin() + below(other.size() + 1), other.end()); break;   // the other encoding's tail
        default: m.insert(m.end(), (size_t)(1 + below(64)), (uint8_t)rnd()); break;                                              // padding
    }
    return m;
}

int main(int argc, char **argv) {
    if (argc != 5) { fprintf(stderr, "usage: keyfile_fuzz raw.bin compressed.bin iterations seed\n"); return 2; }
    const Bytes seeds[2] = {read_file(argv[1]), read_file(argv[2])};
    const unsigned long iters = strtoul(argv[3], nullptr, 10);
    rng_state = strtoull(argv[4], nullptr, 10);
    mi_pk_raw_info info[2];
    uint32_t enc[2];
    for (int k = 0; k < 2; k++)
        if (!run(seeds[k], &info[k], &enc[k]) || enc[k] != (uint32_t)k) { fprintf(stderr, "keyfile_fuzz: seed file %d is not accepted in its encoding\n", k); return 2; }
    if (info[0].nb_wires != info[1].nb_wires || info[0].n_g1_z != info[1].n_g1_z || info[0].n_g2_b != info[1].n_g2_b || info[0].n_commitment_keys != info[1].n_commitment_keys)
        { fprintf(stderr, "keyfile_fuzz: the two seeds are not one key\n"); return 2; }
    // null pointers are refused, not read
    uint32_t e;
    if (mi_pk_stream_inspect(nullptr, 0, &info[0], &e) == MI_OK || mi_pk_stream_inspect(seeds[0].data(), seeds[0].size(), nullptr, &e) == MI_OK ||
        mi_pk_stream_inspect(seeds[0].data(), seeds[0].size(), &info[0], nullptr) == MI_OK) broken("a null pointer was accepted");
    n_accept = n_refuse = 0;
    for (int k = 0; k < 2; k++) {
        const size_t n = seeds[k].size(), step = n > 6000 ? n / 3000 : 1;
        for (size_t cut = 0; cut < n; cut += step) {
            Bytes m(seeds[k].begin(), seeds[k].begin() + cut);
            if (run(m, &info[0], &e)) broken("a truncated stream was accepted");
        }
    }
    for (unsigned long it = 0; it < iters; it++) {
        const int k = (int)below(2);
        Bytes m = mutate(seeds[k], seeds[1 - k]);
        if (below(8) == 0) m = mutate(m, seeds[k]);
        (void)run(m, &info[0], &e);
    }
    printf("%lu %lu\n", n_accept, n_refuse);
    return 0;
}
