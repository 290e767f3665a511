// The sub-AIR examples of include/cstark.hpp prove and verify: MerkleExample, RangeProofExample and RescueExample accept their own
// proofs, reject them against another statement (VerifierError, verdict OOD) and reject a proof of another AIR (UNSUPPORTED); a
// SchnorrAir proof has no verifier (UNSUPPORTED through cstark_air_verify).  Prints one line per check; exit code 0 = all held.
#include <cstdio>
#include "cstark.hpp"

template <class Example> static int rejected(const Example &ex, const std::vector<uint8_t> &proof) {
    try {
        ex.verify(proof);
    } catch (const cstark::VerifierError &e) {
        return e.verdict;
    }
    return CSTARK_PROOF_OK;
}

int main() {
    int failures = 0;
    auto expect = [&](const char *what, int got, int want) {
        printf("%s: verdict %d (expected %d)\n", what, got, want);
        failures += got != want;
    };
    try {
        cstark::Context ctx;
        const cstark::ProofOptions o4(8, 4, 0, cstark::HashFunction::Blake3_256, cstark::FieldExtension::None, 4, 128);
        const cstark::ProofOptions o8(10, 8, 0, cstark::HashFunction::Sha3_256, cstark::FieldExtension::Quadratic, 8, 128);

        cstark::MerkleExample merkle(o8, cstark::TransactionMetadata::build_random(2, 3, 11), ctx);
        const std::vector<uint8_t> mp = merkle.prove();
        expect("merkle", rejected(merkle, mp), CSTARK_PROOF_OK);
        cstark::MerkleExample other(o8, cstark::TransactionMetadata::build_random(2, 3, 12), ctx);
        expect("merkle, another statement", rejected(other, mp), CSTARK_PROOF_OOD);

        const cstark::BaseElement seventeen = (cstark::BaseElement)((((unsigned __int128)17) << 64) % ((((unsigned __int128)1) << 62) + (((unsigned __int128)1) << 56) + (((unsigned __int128)1) << 55) + 1));
        cstark::RangeProofExample range(o4, seventeen, ctx);   // 64 rows at blowup 4, remainder 128: one FRI layer
        const std::vector<uint8_t> rp = range.prove();
        expect("range", rejected(range, rp), CSTARK_PROOF_OK);
        expect("range, another number", rejected(cstark::RangeProofExample(o4, seventeen + 1, ctx), rp), CSTARK_PROOF_OOD);
        expect("range, a merkle proof", rejected(range, mp), CSTARK_PROOF_UNSUPPORTED);

        cstark::RescueExample rescue(8, o4, ctx);
        const std::vector<uint8_t> cp = rescue.prove();
        expect("rescue", rejected(rescue, cp), CSTARK_PROOF_OK);
        cstark::RescueExample longer(16, o4, ctx);
        expect("rescue, another chain", rejected(longer, cp), CSTARK_PROOF_OOD);

        cstark::SchnorrExample schnorr(cstark::ProofOptions(8, 8, 0, cstark::HashFunction::Blake3_256, cstark::FieldExtension::None, 4, 128), 1, ctx);
        const std::vector<uint8_t> sp = schnorr.prove();
        const uint8_t *ptr = sp.data();
        const size_t len = sp.size();
        const int32_t air = CSTARK_AIR_SCHNORR;
        const uint64_t pub[14] = {};
        int32_t v = -1;
        cstark::check(cstark_air_verify(ctx.raw(), 1, &ptr, &len, &air, pub, nullptr, &v));
        expect("schnorr", v, CSTARK_PROOF_UNSUPPORTED);
    } catch (const std::exception &e) {
        fprintf(stderr, "error: %s\n", e.what());
        return 2;
    }
    return failures ? 1 : 0;
}
