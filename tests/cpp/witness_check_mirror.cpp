// Exercises cstark::check_witness and cstark::check_resident_witness (include/cstark.hpp) the way a host that built its own witness
// would: every witness of a case file is checked in the host form, with signatures and folds; one whose length is a power of two is
// also loaded (TransactionProver::load) and checked where it lies, which must give the same answer.
// usage: witness_check_mirror <cases> <out>
//   <cases>: little-endian u64 words: count, then per witness: depth, n_tx, initial_roots [n][7], final_root [7], s_old_values [n][14],
//            r_old_values [n][14], s_indices [n], r_indices [n], s_paths [n][depth + 1][7], r_paths likewise, deltas [n], sig_rx [n][6],
//            sig_s as [n][4] words
//   <out>:   per witness: n_tx, depth, first_bad (two's complement), first_verdict, n_bad, final_root [7], verdicts [n] (one word each),
//            folds [n][4][7]
// prints "witnesses=<count> resident=<how many were also checked resident> same=<how many of those agreed>"
#include <cstdio>
#include <cstring>
#include <fstream>
#include "cstark.hpp"

static std::vector<uint64_t> read_words(const char *path) {
    std::ifstream f(path, std::ios::binary | std::ios::ate);
    if (!f) throw std::runtime_error(std::string("cannot read ") + path);
    std::vector<uint64_t> words((size_t)f.tellg() / 8);
    f.seekg(0);
    f.read((char *)words.data(), (std::streamsize)(8 * words.size()));
    return words;
}

int main(int argc, char **argv) {
    if (argc < 3) return 2;
    try {
        const std::vector<uint64_t> in = read_words(argv[1]);
        std::vector<uint64_t> out;
        size_t at = 0;
        auto take = [&](void *dst, size_t words) {
            if (at + words > in.size()) throw std::runtime_error("the case file is short");
            std::memcpy(dst, in.data() + at, 8 * words);
            at += words;
        };
        uint64_t count = 0;
        take(&count, 1);
        cstark::Context ctx;
        unsigned resident = 0, same = 0;
        for (uint64_t k = 0; k < count; k++) {
            uint64_t depth = 0, n = 0;
            take(&depth, 1);
            take(&n, 1);
            cstark::TransactionMetadata m;
            m.merkle_depth = (unsigned)depth;
            m.initial_roots.resize(n); m.s_old_values.resize(n); m.r_old_values.resize(n); m.s_indices.resize(n); m.r_indices.resize(n);
            m.s_paths.resize(n * (depth + 1) * 7); m.r_paths.resize(n * (depth + 1) * 7); m.deltas.resize(n); m.sig_rx.resize(n); m.sig_s.resize(n);
            take(m.initial_roots.data(), 7 * n); take(m.final_root.data(), 7); take(m.s_old_values.data(), 14 * n); take(m.r_old_values.data(), 14 * n);
            take(m.s_indices.data(), n); take(m.r_indices.data(), n); take(m.s_paths.data(), m.s_paths.size()); take(m.r_paths.data(), m.r_paths.size());
            take(m.deltas.data(), n); take(m.sig_rx.data(), 6 * n); take(m.sig_s.data(), 4 * n);
            const cstark::WitnessCheck got = cstark::check_witness(ctx, m, true, true);
            if (got.ok() != (got.report.n_bad == 0) || got.verdicts.size() != n || got.folds.size() != 28 * n) throw std::runtime_error("inconsistent result");
            const cstark_witness_report &r = got.report;
            out.insert(out.end(), {r.n_tx, r.merkle_depth, (uint64_t)(int64_t)r.first_bad, r.first_verdict, r.n_bad});
            out.insert(out.end(), r.final_root, r.final_root + 7);
            out.insert(out.end(), got.verdicts.begin(), got.verdicts.end());
            out.insert(out.end(), got.folds.begin(), got.folds.end());
            if ((n & (n - 1)) == 0) {
                cstark::TransactionProver prover(cstark::ProofOptions(), ctx);
                prover.load(m);
                const cstark::WitnessCheck lies = cstark::check_resident_witness(ctx, n, &m.final_root, true, true);
                resident++;
                same += lies.verdicts == got.verdicts && lies.folds == got.folds && std::memcmp(&lies.report, &got.report, sizeof got.report) == 0;
            }
        }
        std::ofstream f(argv[2], std::ios::binary);
        f.write((const char *)out.data(), (std::streamsize)(8 * out.size()));
        std::printf("witnesses=%llu resident=%u same=%u\n", (unsigned long long)count, resident, same);
        return 0;
    } catch (const std::exception &e) {
        std::fprintf(stderr, "%s\n", e.what());
        return 3;
    }
}
