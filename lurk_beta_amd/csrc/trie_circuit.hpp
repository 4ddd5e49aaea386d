// trie_circuit.hpp - the R1CS rows of the trie coprocessor's two step circuits, recorded on the host from the slot gadgets' own rows.
//
// LookupCoprocessor and InsertCoprocessor are NIVC step circuits whose bodies are Trie::synthesize_lookup
// (/root/reference/src/coprocessor/trie/mod.rs:652-714) and Trie::synthesize_insert (:802-880); this is what the two functions allocate
// and enforce, given `allocated_root`, `key` (and `value`).  The wrappers around them (synthesize_*_aux: the allocated_root_value
// allocation, implies_equal under not_dummy, the AllocatedPtr tags, the globals) stay with the host and arrive as extra rows.
// Arity 8, height H = 1 .. 85.  Both inner gadgets are the slot gadgets of slot_circuit.hpp, RELOCATED, not derived again.
//
// Lookup block, local columns in allocation order (size_lookup = 1 + B + 403 H; B = the bit-decomposition slot's block size):
//   0                  allocated_root
//   1 .. B             the bit-decomposition slot block of the key (synthesize_path, :611-629: key.to_bits_le_strict)
//   L_i = 1 + B + 403 i, level i = 0 .. H - 1, root level first (synthesize_lookup_at_path, :668-714):
//     L_i .. L_i + 395   the hash8 slot block of path preimage i: [8 preimage | 387 S-box aux | digest]
//     L_i + 396 .. + 402 the seven picks of select (/root/reference/src/circuit/gadgets/constraints.rs:334-391): three rounds of 4, 2 and
//                        1 picks; round r takes the digit's bit 2 - r as condition and pick (r, j) takes a = state[half + j], b = state[j],
//                        the state being the preimage in round 0 and the previous round's picks afterwards
//   The digit of level i is key bits 3 (H - 1 - i) .. + 2 (:611-629); bits at and above the field's NUM_BITS are Boolean::Constant(false)
//   (BN254 at H = 85 only: bit 254, the top bit of level 0's digit).  `found` = the last pick of level H - 1.
// Lookup rows, emission order (rows_lookup = Rb + 396 H; Rb = the bit-decomposition slot's rows):
//   the bit-decomposition slot's rows; then per level the 388 hash8 slot rows, hashed * 1 = next (enforce_equal, constraints.rs:14-31;
//   next = the root at level 0, the previous level's last pick afterwards) and seven pick rows (b - a) * cond = (b - c), B an empty row
//   where cond is the constant false.
// Insert = the lookup block and rows (synthesize_insert_at_path, :820-844, runs the lookup first), then one column for the new value and,
// from the leaf level upward (synthesize_modify_value_at_path, :846-880), the hash8 slot block and rows of that level's new preimage:
//   size_insert = size_lookup + 1 + 396 H, rows_insert = Rb + 784 H; the result is the last digest.
// As in the reference, NOTHING constrains the entries of a new preimage to equal the old preimage's untouched entries or the entry on the
// path to equal the value or the digest below: synthesize_modify_value_at_path allocates them with those values and enforces no row.
// Columns ascend within a row, no zero coefficient, an empty linear combination is an empty CSR row; local column `size` is ONE.
#pragma once
#include <algorithm>
#include <utility>

#include "slot_circuit.hpp"

namespace lurk {

constexpr int TRIE_CIRCUIT_MAX_HEIGHT = 85;
constexpr size_t TRIE_CIRCUIT_HASH_BLOCK = 396, TRIE_CIRCUIT_PICKS = 7;

struct TrieCircuitDims {
    size_t key_block = 0, key_rows = 0;            // B, Rb
    size_t size_lookup = 0, size = 0, num_cons = 0;
    size_t result_col = 0, value_col = 0;          // value_col: insert only
    size_t level(size_t i) const { return 1 + key_block + (TRIE_CIRCUIT_HASH_BLOCK + TRIE_CIRCUIT_PICKS) * i; }
    size_t new_level(size_t k) const { return size_lookup + 1 + TRIE_CIRCUIT_HASH_BLOCK * k; }  // k = 0 is the leaf
};

inline TrieCircuitDims trie_circuit_dims(const SlotCircuit& bits, const SlotCircuit& hash8, int height, bool insert) {
    TrieCircuitDims d;
    const size_t H = (size_t)height;
    d.key_block = bits.size;
    d.key_rows = bits.num_cons;
    d.size_lookup = 1 + d.key_block + (TRIE_CIRCUIT_HASH_BLOCK + TRIE_CIRCUIT_PICKS) * H;
    d.size = insert ? d.size_lookup + 1 + TRIE_CIRCUIT_HASH_BLOCK * H : d.size_lookup;
    d.num_cons = d.key_rows + (hash8.num_cons + 1 + TRIE_CIRCUIT_PICKS) * H + (insert ? hash8.num_cons * H : 0);
    d.value_col = d.size_lookup;
    d.result_col = insert ? d.new_level(H - 1) + TRIE_CIRCUIT_HASH_BLOCK - 1 : d.level(H - 1) + TRIE_CIRCUIT_HASH_BLOCK + TRIE_CIRCUIT_PICKS - 1;
    return d;
}

// the rows of `slot` appended with its block at column `at` and its ONE at column `one` (above every block column: the order within a
// row is kept)
inline void append_relocated(SlotCircuit& out, const SlotCircuit& slot, size_t at, size_t one) {
    for (int w = 0; w < 3; w++) {
        const SlotMatrix& m = slot.m[w];
        SlotMatrix& o = out.m[w];
        const size_t nnz0 = o.indices.size();
        for (uint64_t col : m.indices) o.indices.push_back(col == slot.size ? one : at + col);
        o.data.insert(o.data.end(), m.data.begin(), m.data.end());
        for (size_t r = 1; r < m.indptr.size(); r++) o.indptr.push_back(nnz0 + m.indptr[r]);
    }
    out.num_cons += slot.num_cons;
}

template <class P>
struct TrieRowWriter {
    typedef std::vector<std::pair<size_t, Fe<P>>> LC;  // a few entries, in any order
    SlotCircuit& out;
    void lc(int w, LC l) {
        std::sort(l.begin(), l.end(), [](const auto& a, const auto& b) { return a.first < b.first; });
        SlotMatrix& m = out.m[w];
        for (auto& e : l) {
            m.indices.push_back(e.first);
            for (int i = 0; i < 4; i++) m.data.push_back((uint64_t)e.second.l[2 * i] | ((uint64_t)e.second.l[2 * i + 1] << 32));
        }
        m.indptr.push_back(m.indices.size());
    }
    void enforce(const LC& a, const LC& b, const LC& c) {
        lc(0, a);
        lc(1, b);
        lc(2, c);
        out.num_cons++;
    }
};

// bits, hash8: the bit-decomposition and hash8 slot circuits of the field
template <class P>
SlotCircuit trie_circuit(const SlotCircuit& bits, const SlotCircuit& hash8, int height, bool insert) {
    typedef typename TrieRowWriter<P>::LC LC;
    const TrieCircuitDims d = trie_circuit_dims(bits, hash8, height, insert);
    const size_t H = (size_t)height, one_col = d.size;
    SlotCircuit out;
    out.size = d.size;
    TrieRowWriter<P> cs{out};
    const Fe<P> one = fe_one<P>(), minus_one = fe_neg<P>(fe_one<P>());
    // the key's bits: the unpacking row (the slot's last) lists them by ascending column = from the top bit down
    const SlotMatrix& ba = bits.m[0];
    const size_t num_bits = ba.indptr[bits.num_cons] - ba.indptr[bits.num_cons - 1];
    const uint64_t* bit_cols_be = &ba.indices[ba.indptr[bits.num_cons - 1]];
    append_relocated(out, bits, 1, one_col);
    for (size_t i = 0; i < H; i++) {
        const size_t at = d.level(i), digest = at + TRIE_CIRCUIT_HASH_BLOCK - 1, picks = at + TRIE_CIRCUIT_HASH_BLOCK;
        append_relocated(out, hash8, at, one_col);
        const size_t next = i == 0 ? 0 : d.level(i - 1) + TRIE_CIRCUIT_HASH_BLOCK + TRIE_CIRCUIT_PICKS - 1;
        cs.enforce({{digest, one}}, {{one_col, one}}, {{next, one}});
        size_t state = at, c = picks;  // the first column of the current state, the next pick
        for (size_t r = 0, half = 4; r < 3; r++, half /= 2) {
            const size_t bit = 3 * (H - 1 - i) + (2 - r);
            LC cond;  // Boolean::Constant(false) is an empty combination
            if (bit < num_bits) cond.push_back({1 + (size_t)bit_cols_be[num_bits - 1 - bit], one});
            const size_t first_pick = c;
            for (size_t j = 0; j < half; j++, c++) {
                const size_t a = state + half + j, b = state + j;
                cs.enforce({{b, one}, {a, minus_one}}, cond, {{b, one}, {c, minus_one}});
            }
            state = first_pick;
        }
    }
    if (insert)
        for (size_t k = 0; k < H; k++) append_relocated(out, hash8, d.new_level(k), one_col);
    return out;
}

}  // namespace lurk
