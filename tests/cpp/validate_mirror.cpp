// Exercises cstark::TraceReport, cstark::validate_trace and validate() of the five example classes (include/cstark.hpp): per AIR the
// example's own validate() on its honest witness, then the same trace built into a device buffer, one cell of it raised by 1 and
// validated again without a boundary check.
// usage: validate_mirror <out_prefix>      per AIR a writes <prefix>.a.trace ([width][n] u64, the honest trace), <prefix>.a.codes (u32 per
//        cycle) and <prefix>.a.frame (u64 per constraint) of the corrupted trace; SchnorrAir also <prefix>.2.messages / .rx; prints per
//        AIR one line "air=a clean=<str> ok=<0|1> | step constraint bad_cycles boundary | <str>"
#include <cstdio>
#include <fstream>
#include <functional>
#include "cstark.hpp"

using cstark::BaseElement;

static void dump(const std::string &path, const void *p, size_t n) {
    std::ofstream f(path, std::ios::binary);
    f.write((const char *)p, (std::streamsize)n);
}
static const unsigned __int128 P = ((unsigned __int128)1 << 62) + ((unsigned __int128)1 << 56) + ((unsigned __int128)1 << 55) + 1;
static BaseElement mont(uint64_t v) { return (BaseElement)((((unsigned __int128)v) << 64) % P); }

// the honest trace through `build`, dumped; cell (col, row) + 1; the report of the corrupted trace
static cstark::TraceReport corrupted(cstark::Context &ctx, const std::string &prefix, int air, uint32_t width, size_t n, uint32_t item, uint32_t col, size_t row,
                                     const std::function<int(uint64_t *)> &build) {
    uint32_t log_n = 0;
    while (((size_t)1 << log_n) < n) log_n++;
    void *d = nullptr;
    cstark::check(cstark_malloc(ctx.raw(), (size_t)width * n * 8, &d));
    cstark::check(build((uint64_t *)d));
    std::vector<uint64_t> host((size_t)width * n);
    cstark::check(cstark_memcpy_d2h(ctx.raw(), host.data(), d, host.size() * 8));
    dump(prefix + "." + std::to_string(air) + ".trace", host.data(), host.size() * 8);
    const uint64_t cell = (uint64_t)(((unsigned __int128)host[(size_t)col * n + row] + mont(1)) % P);
    cstark::check(cstark_memcpy_h2d(ctx.raw(), (uint64_t *)d + (size_t)col * n + row, &cell, 8));
    const cstark::TraceReport r = cstark::validate_trace(ctx, air, (const uint64_t *)d, log_n, item, nullptr, true, true);
    cstark_free(ctx.raw(), d);
    dump(prefix + "." + std::to_string(air) + ".codes", r.cycle_codes.data(), 4 * r.cycle_codes.size());
    dump(prefix + "." + std::to_string(air) + ".frame", r.frame_values.data(), 8 * r.frame_values.size());
    return r;
}
static void line(int air, const cstark::TraceReport &clean, const cstark::TraceReport &bad) {
    std::printf("air=%d clean=%s ok=%d | %lld %u %u %d | %s\n", air, clean.str().c_str(), (int)clean.ok(), (long long)bad.step, bad.constraint, bad.bad_cycles,
                bad.boundary, bad.str().c_str());
}

int main(int argc, char **argv) {
    if (argc < 2) return 2;
    const std::string prefix = argv[1];
    try {
        cstark::Context ctx;
        const cstark::ProofOptions opt(8, 8, 0, cstark::HashFunction::Blake3_256, cstark::FieldExtension::None, 4, 128);
        {
            cstark::TransactionExample ex(opt, 2, ctx, 3, 0x5EED);
            const cstark::TraceReport clean = ex.validate(true, true); // leaves the witness resident
            line(0, clean, corrupted(ctx, prefix, 0, 94, 2048, 3, 60, 100, [&](uint64_t *d) { return cstark_tx_build_trace(ctx.raw(), d); }));
            cstark::MerkleExample mx(opt, ex.metadata(), ctx);
            const cstark::TraceReport mclean = mx.validate(true, true);
            line(1, mclean, corrupted(ctx, prefix, 1, 65, 1024, 3, 60, 512, [&](uint64_t *d) { return cstark_merkle_build_trace(ctx.raw(), d); }));
        }
        {
            cstark::SchnorrExample sx(opt, 2, ctx, 9);
            const cstark::TraceReport clean = sx.validate(true, true); // leaves the statement resident
            dump(prefix + ".2.messages", sx.messages.data(), 8 * sx.messages.size());
            dump(prefix + ".2.rx", sx.sig_rx.data(), 8 * sx.sig_rx.size());
            line(2, clean, corrupted(ctx, prefix, 2, 56, 1024, 0, 7, 511, [&](uint64_t *d) { return cstark_schnorr_build_trace(ctx.raw(), d); }));
        }
        {
            const BaseElement number = mont(12345);
            cstark::RangeProofExample rx(opt, number, ctx);
            line(3, rx.validate(true, true), corrupted(ctx, prefix, 3, 2, 64, 0, 0, 7, [&](uint64_t *d) { return cstark_range_build_trace(ctx.raw(), number, d); }));
        }
        {
            cstark::RescueExample cx(16, opt, ctx);
            line(4, cx.validate(true, true),
                 corrupted(ctx, prefix, 4, 14, 128, 0, 3, 8, [&](uint64_t *d) { return cstark_rescue_chain_build_trace(ctx.raw(), cx.seed, 16, d); }));
        }
        return 0;
    } catch (const std::exception &e) {
        std::fprintf(stderr, "%s\n", e.what());
        return 3;
    }
}
