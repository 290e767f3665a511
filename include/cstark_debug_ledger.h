/* cstark_debug_ledger.h -- TEST-ONLY, served by libcstark_debug.so like cstark_debug_commit.h: a thin wrapper over an internal host
 * function of the product library (ledger_xor_word, csrc/ledger.hip).  Nothing of the public interface can make a resident account
 * tree inconsistent; the tests of cstark_ledger_audit need a tree that is.
 */
#ifndef CSTARK_DEBUG_LEDGER_H
#define CSTARK_DEBUG_LEDGER_H
#include <stdint.h>
#ifdef __cplusplus
extern "C" {
#endif
#define CSTARK_DEBUG_LEDGER_EMPTY 0xFFFFFFFFu /* as `level`: `index` names an empty-subtree digest (0 .. depth) instead of a node */
/* XORs `mask` into word `word` (0 .. 6) of the digest that the lookup at checkpoint `id` (0: the current state) finds for node
 * (level, index): level 0 = the root, level depth = the leaves.  The digest is changed where it is stored, so every state that shares
 * the slot sees the change, and the same call again undoes it.  `ledger` is a cstark_ledger.  One word is copied down and up; nothing
 * is launched.  Return: 0 = done; 1 (hipErrorInvalidValue) = refused, nothing written: a null or broken ledger, an id that is not live,
 * a node the state does not store (it reads an empty-subtree digest: name that one with CSTARK_DEBUG_LEDGER_EMPTY), a level, index or
 * word out of range; any other value is the hipError_t of a failed runtime call. */
int cstark_debug_ledger_xor_word(void *ledger, uint64_t id, uint32_t level, uint64_t index, uint32_t word, uint64_t mask);
#ifdef __cplusplus
}
#endif
#endif
