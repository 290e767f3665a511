// The reference's acceptance tests (src/tests.rs:11-38) through include/cstark.hpp: prove 2 transfers, verify the proof, then verify a
// tampered copy and catch cstark::VerifierError.  Prints "accepted=1 rejected=<verdict> batch=<v0>,<v1>" on success.
#include <cstdio>
#include "cstark.hpp"

int main() {
    try {
        cstark::Context ctx;
        cstark::ProofOptions options(42, 8, 0, cstark::HashFunction::Blake3_256, cstark::FieldExtension::None, 4, 256);
        cstark::TransactionExample transaction(options, 2, ctx, /*depth=*/3, /*seed=*/0x5EED);
        const std::vector<uint8_t> proof = transaction.prove();
        transaction.verify(proof); // throws on rejection
        std::vector<uint8_t> bad = proof;
        bad[bad.size() - 20] ^= 0x08; // a remainder word
        int rejected = -1;
        try {
            transaction.verify(bad);
        } catch (const cstark::VerifierError &e) {
            rejected = e.verdict;
        }
        const std::vector<int32_t> v = cstark::verify_batch(ctx, {proof, bad}, {transaction.pub_inputs(), transaction.pub_inputs()}, &options);
        std::printf("accepted=1 rejected=%d batch=%d,%d\n", rejected, v[0], v[1]);
        return rejected > 0 && v[0] == CSTARK_PROOF_OK && v[1] == rejected ? 0 : 1;
    } catch (const std::exception &e) {
        std::printf("error: %s\n", e.what());
        return 1;
    }
}
