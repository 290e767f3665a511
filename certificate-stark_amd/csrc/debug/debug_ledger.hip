// A stored digest of an account ledger, changed by a test (include/cstark_debug_ledger.h): the product's own host function behind one
// exported name.  Every check is ledger_xor_word's (csrc/ledger.hip).
#include <hip/hip_runtime.h>
#include "../../../include/cstark_debug_ledger.h"
#include "../ctx.h"

extern "C" int cstark_debug_ledger_xor_word(void *ledger, uint64_t id, uint32_t level, uint64_t index, uint32_t word, uint64_t mask) {
    return ledger_xor_word((cstark_ledger *)ledger, id, level, index, word, mask);
}
