// The compact proof form through include/cstark.hpp: a context set to CSTARK_FORM_COMPACT proves MerkleAir, RangeProofAir and RescueAir
// statements whose proofs carry the compact magic, are shorter than the plain proofs of the same statements, agree with them up to the
// end of the trace rows (but for the magic) and verify; a damaged multiproof node is a TRACE_OPENING; back in the plain form the context
// writes the plain bytes again.  Prints one line per check; exit code 0 = all held.
#include <cstdio>
#include <cstring>
#include "cstark.hpp"

template <class Example> static int verdict_of(const Example &ex, const std::vector<uint8_t> &proof) {
    try {
        ex.verify(proof);
    } catch (const cstark::VerifierError &e) {
        return e.verdict;
    }
    return CSTARK_PROOF_OK;
}

int main() {
    int failures = 0;
    auto expect = [&](const char *what, long got, long want) {
        printf("%s: %ld (expected %ld)\n", what, got, want);
        failures += got != want;
    };
    try {
        cstark::Context ctx;
        expect("default form", ctx.proof_form(), CSTARK_FORM_PLAIN);
        const cstark::ProofOptions o4(8, 4, 0, cstark::HashFunction::Blake3_256, cstark::FieldExtension::None, 4, 128);
        const cstark::ProofOptions o8(10, 8, 0, cstark::HashFunction::Sha3_256, cstark::FieldExtension::Quadratic, 8, 128);
        cstark::MerkleExample merkle(o8, cstark::TransactionMetadata::build_random(2, 3, 11), ctx);
        const cstark::BaseElement seventeen = (cstark::BaseElement)((((unsigned __int128)17) << 64) % ((((unsigned __int128)1) << 62) + (((unsigned __int128)1) << 56) + (((unsigned __int128)1) << 55) + 1));
        cstark::RangeProofExample range(o4, seventeen, ctx);
        cstark::RescueExample rescue(8, o4, ctx);

        const std::vector<uint8_t> mp = merkle.prove(), rp = range.prove(), cp = rescue.prove();
        ctx.set_proof_form(CSTARK_FORM_COMPACT);
        expect("form after set", ctx.proof_form(), CSTARK_FORM_COMPACT);
        const std::vector<uint8_t> mc = merkle.prove(), rc = range.prove(), cc = rescue.prove();
        ctx.set_proof_form(CSTARK_FORM_PLAIN);
        expect("plain again: same bytes", merkle.prove() == mp && range.prove() == rp && rescue.prove() == cp, 1);
        bool refused = false;
        try { ctx.set_proof_form(2); } catch (const cstark::Error &) { refused = true; }
        expect("form 2 refused", refused && ctx.proof_form() == CSTARK_FORM_PLAIN, 1);

        const std::vector<uint8_t> *plain[3] = {&mp, &rp, &cp}, *compact[3] = {&mc, &rc, &cc};
        const size_t widths[3] = {65, 2, 14};
        for (int i = 0; i < 3; i++) {
            const std::vector<uint8_t> &p = *plain[i], &c = *compact[i];
            expect("plain magic", cstark::proof_form(p), CSTARK_FORM_PLAIN);
            expect("compact magic", cstark::proof_form(c), CSTARK_FORM_COMPACT);
            expect("compact is shorter", c.size() < p.size(), 1);
            // header words .. trace rows: 52 + 64 + 4 + 32 layers + 32 + frame + 8 + rows; compare a prefix that every shape here has
            const size_t head = 52 + 64 + 4 + 32 + 8 * widths[i];
            expect("same bytes behind the magic", memcmp(p.data() + 4, c.data() + 4, head - 4) == 0, 1);
        }
        expect("merkle compact", verdict_of(merkle, mc), CSTARK_PROOF_OK);
        expect("range compact", verdict_of(range, rc), CSTARK_PROOF_OK);
        expect("rescue compact", verdict_of(rescue, cc), CSTARK_PROOF_OK);
        expect("range compact, another number", verdict_of(cstark::RangeProofExample(o4, seventeen + 1, ctx), rc), CSTARK_PROOF_OOD);

        // the first node of the range proof's trace multiproof: 64 rows at blowup 4 -> 256 points, remainder 128, folding 4: one layer;
        // the trace rows end at 52 + 64 + 4 + 32 + 32 + 8 (2 * 2 + 2) + 8 + 8 * 8 * 2, then the count word
        std::vector<uint8_t> bad = rc;
        const size_t nodes = 52 + 64 + 4 + 32 + 32 + 8 * 6 + 8 + 8 * 8 * 2 + 4;
        bad[nodes + 5] ^= 0x10;
        expect("range compact, a damaged trace node", verdict_of(range, bad), CSTARK_PROOF_TRACE_OPENING);

        bool threw = false;
        try { cstark::proof_form(std::vector<uint8_t>{'C', 'S', 'T', 'X', 0, 0}); } catch (const cstark::Error &) { threw = true; }
        expect("unknown magic refused", threw, 1);
    } catch (const std::exception &e) {
        fprintf(stderr, "error: %s\n", e.what());
        return 2;
    }
    return failures ? 1 : 0;
}
