// Mutation driver for the host-only readers of include/mi355x_groth16_vkfile.h: mi_vk_stream_inspect (and mi_vk_stream_size over what
// it reports) and mi_public_witness_read.  Compiled TOGETHER with csrc/vkfile_inspect.hip as plain C++ under
// -fsanitize=address,undefined (gnark-whir_amd/Makefile `sanitize-vkfile`; tests/test_vkfile_cpu.py builds and runs it on the CPU --
// sanitizers belong on this build only).  Test infrastructure.
//
//   vkfile_fuzz <vk_raw.bin> <vk_compressed.bin> <witness.bin> <iterations> <seed>
//
// The three seed files are VALID (the driver first checks that each is accepted, the two key streams in their own encodings with the same
// counts).  Mutations: every truncation, bit flips, byte writes, 4- and 8-byte big-endian counts overwritten with 0, 1, 2^31, 2^32 - 1
// and values near the input's own length, random blobs, splices of one encoding's head onto the other's tail.  Every mutant is copied
// into a heap block of exactly its size, so a read past the input is the sanitizer's to find.  Exit status 0 = no sanitizer report and
// no broken contract: an accepted key stream names fields that lie inside it, one after the other, has the length mi_vk_stream_size
// computes from its counts, and its indices are in range; an accepted witness has the length its header states and its values, written
// back by mi_public_witness_write, are its own bytes.  Prints "accepted refused".
#include "../../include/mi355x_groth16_vkfile.h"
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
    if (!f) { fprintf(stderr, "vkfile_fuzz: cannot open %s\n", path); exit(2); }
    uint8_t buf[65536];
    size_t n;
    while ((n = fread(buf, 1, sizeof buf, f)) > 0) b.insert(b.end(), buf, buf + n);
    fclose(f);
    return b;
}
[[noreturn]] static void broken(const char *what) { fprintf(stderr, "vkfile_fuzz: %s\n", what); exit(3); }

static unsigned long n_accept, n_refuse;

static uint8_t *exact_copy(const Bytes &in) {
    uint8_t *exact = (uint8_t *)malloc(in.size() ? in.size() : 1);   // no slack behind the last byte
    if (!exact) broken("out of memory");
    if (!in.empty()) memcpy(exact, in.data(), in.size());
    return exact;
}

// true = accepted; info and encoding as the library left them
static bool run_vk(const Bytes &in, mi_vk_stream_info *info, uint32_t *encoding) {
    uint8_t *exact = exact_copy(in);
    const int32_t rc = mi_vk_stream_inspect(exact, in.size(), info, encoding);
    if (rc != MI_OK) {
        n_refuse++;
        free(exact);
        if (!memchr(info->refused, 0, sizeof(info->refused))) broken("the refusal's message is not terminated");
        return false;
    }
    n_accept++;
    if (*encoding > MI_KEYFILE_COMPRESSED) broken("an accepted stream has no known encoding");
    const uint64_t g1 = *encoding == MI_KEYFILE_COMPRESSED ? 32 : 64, g2 = 2 * g1;
    uint64_t at = 0;
    auto field = [&](uint64_t off, unsigned __int128 bytes, uint64_t gap) {   // gap: the count in front of it
        if (off != at + gap || (unsigned __int128)off + bytes > in.size()) broken("a field is not where the layout puts it, or leaves the input");
        at = off + (uint64_t)bytes;
    };
    field(info->off_alpha1, g1, 0); field(info->off_beta1, g1, 0); field(info->off_beta2, g2, 0); field(info->off_gamma2, g2, 0);
    field(info->off_delta1, g1, 0); field(info->off_delta2, g2, 0);
    field(info->off_k, (unsigned __int128)info->n_k * g1, 4);
    if (info->off_lists != at) broken("the lists do not follow K");
    if (info->n_commitment_keys > MI_PK_RAW_MAX_COMMITMENTS) broken("more Pedersen keys than the info has room for");
    if (info->n_k < 1 + (uint64_t)info->n_commitment_keys || info->nb_public != info->n_k - info->n_commitment_keys) broken("nb_public is not n_k - n_commitment_keys");
    uint32_t off[MI_PK_RAW_MAX_COMMITMENTS + 1] = {0};
    at += 4;
    for (uint32_t k = 0; k < info->n_commitment_keys; k++) {
        field(info->off_list[k], (unsigned __int128)info->list_len[k] * 8, 4);
        for (uint64_t t = 0; t < info->list_len[k]; t++) {
            uint64_t v = 0;
            for (int s = 0; s < 8; s++) v = (v << 8) | exact[info->off_list[k] + 8 * t + s];
            if (v < 1 || v > (uint64_t)info->nb_public - 1 + k) broken("an accepted stream has an index outside its range");
        }
        off[k + 1] = off[k] + (uint32_t)info->list_len[k];
    }
    if (info->off_commitment_keys != at) broken("the Pedersen keys do not follow the lists");
    at += 4;
    for (uint32_t k = 0; k < info->n_commitment_keys; k++) field(info->off_ped[k], 2 * g2, 0);
    if (at != in.size()) broken("an accepted stream does not end where its last field ends");
    mi_vk_file_desc d;
    memset(&d, 0, sizeof d);
    d.n_k = info->n_k; d.nb_public = info->nb_public; d.n_commitments = info->n_commitment_keys; d.pc_offsets = off;
    size_t len = 0;
    if (mi_vk_stream_size(&d, *encoding, &len) != MI_OK || len != in.size()) broken("mi_vk_stream_size disagrees with an accepted stream's length");
    free(exact);
    return true;
}

static bool run_witness(const Bytes &in) {
    uint8_t *exact = exact_copy(in);
    const size_t cap = in.size() / 32 + 1;
    mi_fr *out = (mi_fr *)malloc(cap * sizeof(mi_fr));
    if (!out) broken("out of memory");
    size_t n = ~(size_t)0;
    const int32_t rc = mi_public_witness_read(exact, in.size(), out, cap, &n);
    if (rc != MI_OK) { n_refuse++; free(exact); free(out); return false; }
    n_accept++;
    if (in.size() < 12 || n > (in.size() - 12) / 32) broken("an accepted witness has more public values than bytes");
    const size_t total = ((size_t)exact[8] << 24) | ((size_t)exact[9] << 16) | ((size_t)exact[10] << 8) | exact[11];
    if (in.size() != 12 + 32 * total) broken("an accepted witness does not have the length its header states");
    Bytes back(12 + 32 * n);
    size_t len = 0;
    if (mi_public_witness_write(out, n, back.data(), back.size(), &len) != MI_OK || len != back.size()) broken("the values read cannot be written");
    if (n && memcmp(back.data() + 12, exact + 12, 32 * n) != 0) broken("the values read, written back, are not the witness's bytes");
    free(exact);
    free(out);
    return true;
}

static void put_be(Bytes &b, size_t at, uint64_t v, int bytes) {
    for (int i = 0; i < bytes; i++)
        if (at + i < b.size()) b[at + i] = (uint8_t)(v >> (8 * (bytes - 1 - i)));
}

static Bytes mutate(const Bytes &seed, const Bytes &other) {
    Bytes b = seed;
    const uint64_t interesting[] = {0, 1, 2, 16, 17, (uint64_t)1 << 31, 0xffffffffull, (uint64_t)1 << 32, ~(uint64_t)0, seed.size(), seed.size() / 32, seed.size() / 64 + 1};
    const int rounds = 1 + (int)below(3);
    for (int r = 0; r < rounds; r++) {
        switch (below(8)) {
        case 0: if (!b.empty()) b[below(b.size())] ^= (uint8_t)(1u << below(8)); break;
        case 1: if (!b.empty()) b[below(b.size())] = (uint8_t)rnd(); break;
        case 2: put_be(b, below(b.size() + 1), interesting[below(sizeof interesting / sizeof *interesting)], 4); break;
        case 3: put_be(b, below(b.size() + 1), interesting[below(sizeof interesting / sizeof *interesting)], 8); break;
        case 4: b.resize(below(b.size() + 1)); break;
        case 5: { const size_t extra = 1 + below(64); for (size_t i = 0; i < extra; i++) b.push_back((uint8_t)rnd()); break; }
        case 6: { const size_t cut = below(b.size() + 1), from = below(other.size() + 1); b.resize(cut); b.insert(b.end(), other.begin() + from, other.end()); break; }
        default: { b.resize(below(200)); for (auto &x : b) x = (uint8_t)rnd(); break; }
        }
    }
    return b;
}

int main(int argc, char **argv) {
    if (argc != 6) { fprintf(stderr, "usage: vkfile_fuzz <vk_raw.bin> <vk_compressed.bin> <witness.bin> <iterations> <seed>\n"); return 2; }
    const Bytes raw = read_file(argv[1]), comp = read_file(argv[2]), wit = read_file(argv[3]);
    const long iters = atol(argv[4]);
    rng_state = (uint64_t)atoll(argv[5]) * 2654435761u + 1;
    mi_vk_stream_info a, b;
    uint32_t ea = 9, eb = 9;
    if (!run_vk(raw, &a, &ea) || ea != MI_KEYFILE_RAW) broken("the raw seed stream is not accepted as raw");
    if (!run_vk(comp, &b, &eb) || eb != MI_KEYFILE_COMPRESSED) broken("the compressed seed stream is not accepted as compressed");
    if (a.n_k != b.n_k || a.n_commitment_keys != b.n_commitment_keys || memcmp(a.list_len, b.list_len, sizeof a.list_len)) broken("the two seed streams differ in their counts");
    if (!run_witness(wit)) broken("the seed witness is not accepted");
    // every strict prefix is refused
    for (const Bytes *s : {&raw, &comp})
        for (size_t cut = 0; cut < s->size(); cut++)
            if (run_vk(Bytes(s->begin(), s->begin() + cut), &a, &ea)) broken("a strict prefix of a key stream is accepted");
    for (size_t cut = 0; cut < wit.size(); cut++)
        if (run_witness(Bytes(wit.begin(), wit.begin() + cut))) broken("a strict prefix of the witness is accepted");
    for (long i = 0; i < iters; i++) {
        switch (below(3)) {
        case 0: run_vk(mutate(raw, comp), &a, &ea); break;
        case 1: run_vk(mutate(comp, raw), &a, &ea); break;
        default: run_witness(mutate(wit, comp)); break;
        }
    }
    printf("%lu %lu\n", n_accept, n_refuse);
    return 0;
}
