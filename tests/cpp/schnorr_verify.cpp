// SchnorrExample of include/cstark.hpp proves and verifies (cstark_schnorr_verify): it accepts its own proofs (one signature in the base
// field; two signatures, Sha3, quadratic extension), rejects them against another statement (VerifierError, verdict OOD -- other
// signatures, and another number of signatures) and rejects a RangeProofAir proof (UNSUPPORTED).  Prints one line per check; exit code
// 0 = all held.
#include <cstdio>
#include "cstark.hpp"

static int rejected(const cstark::SchnorrExample &ex, const std::vector<uint8_t> &proof) {
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
        const cstark::ProofOptions o1(8, 8, 0, cstark::HashFunction::Blake3_256, cstark::FieldExtension::None, 4, 128);
        const cstark::ProofOptions o2(10, 8, 0, cstark::HashFunction::Sha3_256, cstark::FieldExtension::Quadratic, 8, 128);

        cstark::SchnorrExample one(o1, 1, ctx);
        const std::vector<uint8_t> p1 = one.prove();
        expect("schnorr, 1 signature", rejected(one, p1), CSTARK_PROOF_OK);
        cstark::SchnorrExample two(o2, 2, ctx);
        const std::vector<uint8_t> p2 = two.prove();
        expect("schnorr, 2 signatures", rejected(two, p2), CSTARK_PROOF_OK);
        expect("schnorr, other signatures", rejected(cstark::SchnorrExample(o1, 1, ctx, 0xBEEF), p1), CSTARK_PROOF_OOD);
        expect("schnorr, another number of signatures", rejected(two, p1), CSTARK_PROOF_OOD);
        expect("schnorr, half the signatures", rejected(one, p2), CSTARK_PROOF_OOD);

        const cstark::BaseElement seventeen = (cstark::BaseElement)((((unsigned __int128)17) << 64) % ((((unsigned __int128)1) << 62) + (((unsigned __int128)1) << 56) + (((unsigned __int128)1) << 55) + 1));
        const std::vector<uint8_t> rp = cstark::RangeProofExample(o1, seventeen, ctx).prove();
        expect("schnorr, a range proof", rejected(one, rp), CSTARK_PROOF_UNSUPPORTED);
    } catch (const std::exception &e) {
        fprintf(stderr, "error: %s\n", e.what());
        return 2;
    }
    return failures ? 1 : 0;
}
