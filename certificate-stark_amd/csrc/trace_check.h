// Host side of cstark_air_validate_trace: per AIR the shape the frame kernel runs on (width, slots, cycle length, raw
// periodic columns), the boundary list its generic kernel checks, and the decoding of a per-cycle code.  No HIP header: compiles under
// plain g++ (tests/cpp/trace_check_check.cpp).
#pragma once
#include <stdint.h>
#include <vector>
#include "air_groups.h"

namespace cs {

constexpr uint32_t VALIDATE_CLEAN = 0xFFFFFFFFu;
constexpr uint32_t VALIDATE_MAX_LOG_N = 24;
// One boundary entry: register `reg` holds `value` at step `first` (stride 0) or at every step first + k * stride < n; seq >= 0: the
// value of occurrence k is element k of sequence `seq` instead (seq table [n_seq][n / stride]).
struct ValidateEntry {
    uint32_t reg, first, stride;
    int32_t seq;
    uint64_t value;
};

namespace host {

struct TraceCheckShape {
    uint32_t width = 0, nc = 0, n_per = 0;
    uint32_t log_cycle = 0; // log2 of the cycle length (RangeProofAir: the whole trace is one cycle)
};
// false: `air` is no AIR, or it has no trace of 2^log_n rows (fewer rows than one cycle, or more than 2^24)
inline bool trace_check_shape(int air, uint32_t log_n, TraceCheckShape &s) {
    s = TraceCheckShape{};
    if (log_n > VALIDATE_MAX_LOG_N) return false;
    if (air == 0) { s.width = 94; s.nc = 115; s.n_per = 48; s.log_cycle = 10; }
    else if (air == 1) { s.width = 65; s.nc = 106; s.n_per = 33; s.log_cycle = 9; }
    else if (air == 2) { s.width = 56; s.nc = 56; s.n_per = 36; s.log_cycle = 9; }
    else if (air == 3) { s.width = 2; s.nc = 2; s.n_per = 0; s.log_cycle = log_n; return log_n >= 1; }
    else if (air == 4) { s.width = 14; s.nc = 14; s.n_per = 29; s.log_cycle = 3; }
    else return false;
    return log_n >= s.log_cycle;
}
// the depths cstark_ledger_create lists
inline bool trace_check_depth(uint32_t depth) { return depth == 1 || depth == 3 || depth == 7 || depth == 15 || depth == 31; }

// code = (row in cycle) * nc + constraint of cycle `cycle`
struct TraceViolation {
    uint64_t cycle = 0, step = 0;
    uint32_t row_in_cycle = 0, constraint = 0;
};
inline TraceViolation trace_check_decode(const TraceCheckShape &s, uint64_t cycle, uint32_t code) {
    TraceViolation v;
    v.cycle = cycle;
    v.row_in_cycle = code / s.nc;
    v.constraint = code % s.nc;
    v.step = (cycle << s.log_cycle) + v.row_in_cycle;
    return v;
}

// The boundary list of an AIR in the order of cstark_trace_report::boundary.  pub: the 14 public words (RangeProofAir: word 0), unused
// for SchnorrAir, whose sequence values come from sig_rx [n_sig][6] (n_sig * 512 rows): seq receives [12][n_sig], R.x word k of every
// signature at sequences k and 6 + k.  false: not an AIR / a trace length it cannot have.
inline bool trace_check_entries(int air, uint32_t log_n, const uint64_t *pub, const uint64_t *sig_rx, std::vector<ValidateEntry> &entries,
                                std::vector<uint64_t> &seq) {
    TraceCheckShape s;
    entries.clear();
    seq.clear();
    if (!trace_check_shape(air, log_n, s)) return false;
    const uint32_t last = (uint32_t)(((uint64_t)1 << log_n) - 1);
    if (air == 0 || air == 1 || air == 4) { // roots in registers 58..64 / the chain's rate half in registers 0..6: first row, then last row
        const uint32_t r0 = air == 4 ? 0 : 58;
        for (uint32_t a = 0; a < 14; a++) entries.push_back({r0 + a % 7, a < 7 ? 0 : last, 0, -1, pub[a]});
        return true;
    }
    if (air == 3) {
        entries.push_back({1, 0, 0, -1, 0});
        entries.push_back({1, last, 0, -1, pub[0]});
        return true;
    }
    AirShape sh;
    const uint64_t n_sig = ((uint64_t)1 << log_n) / 512;
    if (!air_shape(2, sh, (uint32_t)n_sig)) return false;
    for (size_t a = 0; a < sh.a_reg.size(); a++) entries.push_back({sh.a_reg[a], sh.a_first[a], sh.a_stride[a], sh.a_seq[a], sh.a_const[a]});
    seq.resize(12 * n_sig);
    for (uint64_t q = 0; q < 12; q++)
        for (uint64_t t = 0; t < n_sig; t++) seq[q * n_sig + t] = sig_rx[6 * t + q % 6];
    return true;
}

} // namespace host
} // namespace cs
