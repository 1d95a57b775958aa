// Stand-alone sanitizer run of the locating verifier's descent (gnark-whir_amd/csrc/pairing_ops.cuh, LocateTree and LocatePlan: plain
// host C++, the text verify_locate.hip and the host build of the tests both run): built with -fsanitize=address,undefined
// -DMI_CHECK_NOWRAP by `make sanitize-locate`, run by tests/test_verify_locate_cpu.py.  The flags and every round's answers are heap
// blocks of exactly the size the plan may read, so one byte read too far is a report.  n in {1, 2, 8, 9, 64, 65, 130, 513}, node budgets
// {1, 2, 8, 64}, bad proofs at: the first proof; the last proof (alone in its level-1 node for 9, 65, 513); both; the whole last level-1
// node -- each without malformed proofs and with every third proof that is not bad malformed.  A node fails exactly when it holds a bad
// proof.  Checked: every queried node exists, a round lies on one level below the last one, the suspects are well formed, ascending,
// hold every bad proof and lie in final nodes that hold one, and the counts add up.  Then, per n and budget, answers no exact arithmetic
// gives (the root fails, every child passes): every well-formed proof must stay under suspicion.  Prints the number of descents checked.
#include <cstdio>
#include <cstdlib>
#include <memory>
#include <set>
#include <vector>
#include "../../gnark-whir_amd/csrc/pairing_ops.cuh"

namespace {
unsigned checked = 0;
void require(bool ok, const char *what, size_t n, unsigned cap, int set, int variant) {
    if (ok) return;
    std::printf("FAILED: %s (n %zu, cap %u, set %d, variant %d)\n", what, n, cap, set, variant);
    std::exit(1);
}

void run(size_t n, unsigned cap, int set, int variant, bool children_lie) {
    std::set<size_t> bad;
    if (set == 0 || set == 2) bad.insert(0);
    if (set == 1 || set == 2) bad.insert(n - 1);
    if (set == 3)
        for (size_t i = (n - 1) / 8 * 8; i < n; i++) bad.insert(i);
    std::unique_ptr<uint8_t[]> flags(new uint8_t[n]);
    size_t good = 0;
    for (size_t i = 0; i < n; i++) {
        flags[i] = variant == 1 && i % 3 == 1 && !bad.count(i);
        good += !flags[i];
    }
    LocatePlan plan(n, flags.get(), cap);
    const LocateTree &tree = plan.tree;
    require(tree.cnt[0] == n && tree.cnt[tree.L] == 1 && tree.L >= 1 && tree.off[tree.L] + 1 == tree.total, "shape of the tree", n, cap, set, variant);
    auto holds_bad = [&](u32 l, size_t j) {
        for (size_t i : bad)
            if (i >= tree.first(l, j) && i < tree.end(l, j)) return true;
        return false;
    };
    uint64_t nodes = 0;
    uint32_t rounds = 0;
    u32 last_level = tree.L + 1;
    if (plan.start()) {
        bool more;
        do {
            const size_t m = plan.query.size();
            require(m >= 1 && plan.level < last_level && plan.level >= 1, "a round on one level below the last", n, cap, set, variant);
            require(!plan.parent_end.empty() && plan.parent_end.back() == m, "children grouped by their parents", n, cap, set, variant);
            last_level = plan.level;
            std::unique_ptr<uint8_t[]> pass(new uint8_t[m]);
            for (size_t t = 0; t < m; t++) {
                require(plan.query[t] < tree.cnt[plan.level] && (!t || plan.query[t] > plan.query[t - 1]), "queried nodes exist and ascend", n, cap, set, variant);
                pass[t] = children_lie ? plan.level != tree.L : !holds_bad(plan.level, plan.query[t]);
            }
            nodes += m;
            rounds++;
            more = plan.next(pass.get());
        } while (more);
    }
    const std::vector<size_t> sus = plan.suspects();
    require(plan.stats.rounds == rounds && plan.stats.nodes_tested == nodes && plan.stats.judged_alone == sus.size() && plan.stats.malformed == n - good,
            "counts", n, cap, set, variant);
    for (size_t t = 0; t < sus.size(); t++)
        require(sus[t] < n && !flags[sus[t]] && (!t || sus[t] > sus[t - 1]), "suspects well formed and ascending", n, cap, set, variant);
    if (children_lie) {
        require(sus.size() == good, "children that all pass stay under suspicion", n, cap, set, variant);
        return;
    }
    const std::set<size_t> got(sus.begin(), sus.end());
    for (size_t i : bad) require(got.count(i) == 1, "a bad proof is a suspect", n, cap, set, variant);
    for (size_t i : sus) require(holds_bad(plan.level, i >> (3 * plan.level)), "a suspect's final node holds a bad proof", n, cap, set, variant);
    require(sus.size() <= 8 * bad.size() || plan.level > 1, "a descent to level 1 leaves at most 8 suspects per bad proof", n, cap, set, variant);
    checked++;
}
}   // namespace

int main() {
    for (size_t n : {1, 2, 8, 9, 64, 65, 130, 513})
        for (unsigned cap : {1u, 2u, 8u, 64u}) {
            for (int set = 0; set < 4; set++)
                for (int variant = 0; variant < 2; variant++) run(n, cap, set, variant, false);
            run(n, cap, 0, 0, true);
            run(n, cap, 0, 1, true);
        }
    std::printf("%u\n", checked);
    return 0;
}
