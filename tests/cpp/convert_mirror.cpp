// Conversion between the proof forms through include/cstark.hpp: MerkleAir, RangeProofAir, RescueAir and SchnorrAir statements are
// proved in both forms on one context, and each proof converted to the other form must be the bytes the prover wrote in that form
// (memcmp); a proof already in the target form comes back unchanged; the batch call converts a mix in one launch sequence and refuses a
// damaged proof with the verify call's verdict, without converting it; the bound is the plain length (plus a count word per tree).
// Prints one line per check; exit code 0 = all held.
#include <cstdio>
#include <cstring>
#include "cstark.hpp"

static bool same(const std::vector<uint8_t> &a, const std::vector<uint8_t> &b) {
    return a.size() == b.size() && memcmp(a.data(), b.data(), a.size()) == 0;
}

int main() {
    int failures = 0;
    auto expect = [&](const char *what, long got, long want) {
        printf("%s: %ld (expected %ld)\n", what, got, want);
        failures += got != want;
    };
    try {
        cstark::Context ctx;
        const cstark::ProofOptions o4(8, 4, 0, cstark::HashFunction::Blake3_256, cstark::FieldExtension::None, 4, 128);
        const cstark::ProofOptions o8(10, 8, 0, cstark::HashFunction::Sha3_256, cstark::FieldExtension::Quadratic, 8, 128);
        cstark::MerkleExample merkle(o8, cstark::TransactionMetadata::build_random(2, 3, 11), ctx);
        const cstark::BaseElement seventeen = (cstark::BaseElement)((((unsigned __int128)17) << 64) % ((((unsigned __int128)1) << 62) + (((unsigned __int128)1) << 56) + (((unsigned __int128)1) << 55) + 1));
        cstark::RangeProofExample range(o4, seventeen, ctx);
        cstark::RescueExample rescue(8, o4, ctx);
        cstark::SchnorrExample schnorr(o8, 1, ctx, 91);

        const std::vector<uint8_t> mp = merkle.prove(), rp = range.prove(), cp = rescue.prove(), sp = schnorr.prove();
        ctx.set_proof_form(CSTARK_FORM_COMPACT);
        const std::vector<uint8_t> mc = merkle.prove(), rc = range.prove(), cc = rescue.prove(), sc = schnorr.prove();
        ctx.set_proof_form(CSTARK_FORM_PLAIN);

        expect("merkle plain -> compact", same(merkle.convert(mp), mc), 1);
        expect("merkle compact -> plain", same(merkle.convert(mc, CSTARK_FORM_PLAIN), mp), 1);
        expect("range plain -> compact", same(range.convert(rp), rc), 1);
        expect("range compact -> plain", same(range.convert(rc, CSTARK_FORM_PLAIN), rp), 1);
        expect("rescue plain -> compact", same(rescue.convert(cp), cc), 1);
        expect("rescue compact -> plain", same(rescue.convert(cc, CSTARK_FORM_PLAIN), cp), 1);
        expect("schnorr plain -> compact", same(schnorr.convert(sp), sc), 1);
        expect("schnorr compact -> plain", same(schnorr.convert(sc, CSTARK_FORM_PLAIN), sp), 1);
        expect("already compact: unchanged", same(range.convert(rc), rc), 1);
        expect("already plain: unchanged", same(range.convert(rp, CSTARK_FORM_PLAIN), rp), 1);
        expect("the form setting is not touched", ctx.proof_form(), CSTARK_FORM_PLAIN);

        // the bound: the range proof at blowup 4, remainder 128, folding 4 has one layer -> three trees
        expect("bound to plain", (long)cstark::convert_bound(rc, CSTARK_FORM_PLAIN), (long)rp.size());
        expect("bound to compact", (long)cstark::convert_bound(rp, CSTARK_FORM_COMPACT), (long)rp.size() + 4 * 3);
        bool threw = false;
        try { cstark::convert_bound(std::vector<uint8_t>(rp.begin(), rp.end() - 1), CSTARK_FORM_COMPACT); } catch (const cstark::Error &) { threw = true; }
        expect("no bound for a truncated proof", threw, 1);

        // a damaged trace node (tests/cpp/compact_mirror.cpp: where the first node lies) beside valid proofs, in one call
        std::vector<uint8_t> bad = rc;
        bad[52 + 64 + 4 + 32 + 32 + 8 * 6 + 8 + 8 * 8 * 2 + 4 + 5] ^= 0x10;
        std::array<uint64_t, 14> number{};
        number[0] = seventeen;
        const cstark::Converted got = cstark::air_convert_batch(ctx, {rc, bad, rp}, {CSTARK_AIR_RANGE, CSTARK_AIR_RANGE, CSTARK_AIR_RANGE}, {number, number, number},
                                                                CSTARK_FORM_PLAIN);
        expect("batch: valid compact", got.verdicts[0], CSTARK_PROOF_OK);
        expect("batch: damaged node", got.verdicts[1], CSTARK_PROOF_TRACE_OPENING);
        expect("batch: valid plain", got.verdicts[2], CSTARK_PROOF_OK);
        expect("batch: converted", same(got.proofs[0], rp) && same(got.proofs[2], rp), 1);
        expect("batch: the damaged proof is not converted", (long)got.proofs[1].size(), 0);
        int verdict = CSTARK_PROOF_OK;
        try { range.convert(bad, CSTARK_FORM_PLAIN); } catch (const cstark::VerifierError &e) { verdict = e.verdict; }
        expect("a damaged proof throws its verdict", verdict, CSTARK_PROOF_TRACE_OPENING);
        verdict = CSTARK_PROOF_OK;
        try { cstark::RangeProofExample(o4, seventeen + 1, ctx).convert(rp); } catch (const cstark::VerifierError &e) { verdict = e.verdict; }
        expect("another number: not converted", verdict, CSTARK_PROOF_OOD);
        threw = false;
        try { range.convert(rp, 2); } catch (const cstark::Error &) { threw = true; }
        expect("form 2 refused", threw, 1);
        expect("and the context proves on", same(range.prove(), rp), 1);
    } catch (const std::exception &e) {
        fprintf(stderr, "error: %s\n", e.what());
        return 2;
    }
    return failures ? 1 : 0;
}
