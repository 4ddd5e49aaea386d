// slot_circuit.hpp - the R1CS rows of one slot of a Lurk MultiFrame, recorded on the host from the product's own constants.
//
// The slot-witness kernels (poseidon.hip) write the aux block a slot contributes to W; this is the other half of the same gadgets: the
// constraints that block is allocated for, as (A, B, C) rows over the block's own columns.  Restated from the published algorithms
// (both gadgets live in un-vendored dependencies of the reference, as for the traces - include/lurk_hip.h, "slot witnesses"):
//   neptune circuit2::poseidon_hash_allocated   every S-box input after the first round is a linear combination carried through the
//       linear layers (dense MDS, the pre-sparse matrix, one sparse matrix per partial round); an S-box allocates l^2, l^4, l^5 + key
//       and enforces  l * l = l2,  l2 * l2 = l4,  l4 * l = l5k - key;  the digest is allocated at the end (ensure_allocated):
//       elements[1] * 1 = digest.  3 (t R_F + R_P) + 1 rows.
//   bellpepper to_bits_le_strict   walking the bits of p - 1 from the top: a boolean row (1 - a) a = 0 per 1-bit; a 0-bit closes the open
//       run of 1-bits with an AND chain (cur * next = and) and takes the row (1 - last_run - a) a = 0; the unpacking row
//       (sum 2^i bit_i) * 1 = value closes the gadget.
// Columns: local column k < size is element k of the block as lurk_hip_slot_witness* writes it, local column `size` is the constant ONE.
// Rows in emission order, columns ascending within a row, no zero coefficient, an empty linear combination is an empty CSR row.
// The linear layers are the product's (poseidon_params.hpp: u = Mat s with the sparse rounds [n00, vhat | nw]); the keys are
// neptune_post_keys, the ones the trace kernels add.  Nothing here reads oracle/ - tests/test_slot_constraints.py compares the two.
#pragma once
#include <vector>

#include "poseidon_params.hpp"

namespace lurk {

struct SlotMatrix {
    std::vector<uint64_t> indptr{0}, indices, data;  // data: 4 x u64 per entry, Montgomery(2^256)
};
struct SlotCircuit {
    size_t size = 0, num_cons = 0;  // block elements (ONE is column `size`), rows
    SlotMatrix m[3];
};

// records rows over the dense linear combinations of one block (size + 1 coefficients, most of them zero: blocks are a few hundred long)
template <class P>
struct SlotRecorder {
    typedef std::vector<Fe<P>> LC;
    SlotCircuit out;
    explicit SlotRecorder(size_t size) { out.size = size; }
    size_t one() const { return out.size; }
    LC zero() const { return LC(out.size + 1, fe_zero<P>()); }
    LC var(size_t col) const {
        LC l = zero();
        l[col] = fe_one<P>();
        return l;
    }
    static void add_scaled(LC& acc, const LC& x, const Fe<P>& k) {
        for (size_t i = 0; i < acc.size(); i++)
            if (!fe_is_zero<P>(x[i])) acc[i] = fe_add<P>(acc[i], fe_mul<P>(x[i], k));
    }
    void enforce(const LC& a, const LC& b, const LC& c) {
        const LC* lcs[3] = {&a, &b, &c};
        for (int w = 0; w < 3; w++) {
            SlotMatrix& m = out.m[w];
            for (size_t col = 0; col < lcs[w]->size(); col++) {
                const Fe<P>& v = (*lcs[w])[col];
                if (fe_is_zero<P>(v)) continue;
                m.indices.push_back(col);
                for (int i = 0; i < 4; i++) m.data.push_back((uint64_t)v.l[2 * i] | ((uint64_t)v.l[2 * i + 1] << 32));
            }
            m.indptr.push_back(m.indices.size());
        }
        out.num_cons++;
    }
};

template <class P>
SlotCircuit poseidon_slot_circuit(int arity) {
    typedef typename SlotRecorder<P>::LC LC;
    const PoseidonParams<P> pp = make_poseidon_params<P>(arity);
    const std::vector<Fe<P>> post = neptune_post_keys<P>(pp);
    const int t = pp.t, h = pp.rf / 2;
    SlotRecorder<P> cs((size_t)arity + 3 * ((size_t)t * pp.rf + pp.rp) + 1);
    std::vector<LC> elems(t, cs.zero());
    elems[0][cs.one()] = pp.domain_tag;
    for (int i = 0; i < arity; i++) elems[1 + i] = cs.var(i);
    size_t next = arity;  // the next aux the gadget allocates
    size_t sbox_no = 0;
    auto sbox = [&](const LC& l) {
        const size_t l2 = next, l4 = next + 1, l5 = next + 2;
        next += 3;
        cs.enforce(l, l, cs.var(l2));
        cs.enforce(cs.var(l2), cs.var(l2), cs.var(l4));
        LC c = cs.var(l5);
        c[cs.one()] = fe_neg<P>(post[sbox_no++]);  // l4 * l = l5k - key
        cs.enforce(cs.var(l4), l, c);
        return cs.var(l5);
    };
    auto dense = [&](const std::vector<Fe<P>>& mat) {
        std::vector<LC> u(t, cs.zero());
        for (int j = 0; j < t; j++)
            for (int i = 0; i < t; i++) SlotRecorder<P>::add_scaled(u[j], elems[i], mat[(size_t)j * t + i]);
        elems = u;
    };
    auto full_round = [&](bool first, const std::vector<Fe<P>>& mat) {
        for (int i = 0; i < t; i++) {
            LC l = elems[i];
            if (first) l[cs.one()] = fe_add<P>(l[cs.one()], pp.rc[i]);  // the first round's own constants go in front of its S-boxes
            elems[i] = sbox(l);
        }
        dense(mat);
    };
    for (int r = 0; r < h; r++) full_round(r == 0, r == h - 1 ? pp.pre_sparse : pp.mds);
    for (int p = 0; p < pp.rp; p++) {
        const Fe<P>* sp = &pp.sparse[(size_t)p * (2 * t - 1)];
        const LC x = sbox(elems[0]);
        LC e0 = cs.zero();
        SlotRecorder<P>::add_scaled(e0, x, sp[0]);
        for (int i = 1; i < t; i++) {
            SlotRecorder<P>::add_scaled(e0, elems[i], sp[i]);
            SlotRecorder<P>::add_scaled(elems[i], x, sp[t - 1 + i]);
        }
        elems[0] = e0;
    }
    for (int r = 0; r < h; r++) full_round(false, pp.mds);
    cs.enforce(elems[1], cs.var(cs.one()), cs.var(next));  // ensure_allocated(digest)
    return cs.out;
}

template <class P>
SlotCircuit bit_decomp_slot_circuit() {
    typedef typename SlotRecorder<P>::LC LC;
    uint32_t pm1[8];
    for (int i = 0; i < 8; i++) pm1[i] = P::mod(i);
    pm1[0] -= 1;  // p is odd
    auto bit = [&](int i) { return (pm1[i >> 5] >> (i & 31)) & 1u; };
    // first pass: the walk's allocations (block size), second pass: the rows
    size_t size = 1;
    {
        bool found = false, have_last = false;
        size_t run = 0;
        for (int i = 255; i >= 0; i--) {
            found = found || bit(i);
            if (!found) continue;
            if (bit(i)) {
                run++;
            } else if (run) {
                size += run - 1 + (have_last ? 1 : 0);
                have_last = true;
                run = 0;
            }
            size++;
        }
    }
    SlotRecorder<P> cs(size);
    const Fe<P> minus_one = fe_neg<P>(fe_one<P>());
    size_t next = 1, last = 0;
    bool found = false, have_last = false;
    std::vector<size_t> run, bits_be;
    for (int i = 255; i >= 0; i--) {
        found = found || bit(i);
        if (!found) continue;
        LC a = cs.var(cs.one());
        if (bit(i)) {
            run.push_back(next);
        } else {
            if (!run.empty()) {
                if (have_last) run.push_back(last);
                size_t cur = run[0];
                for (size_t k = 1; k < run.size(); k++) {  // kary_and: one by one
                    cs.enforce(cs.var(cur), cs.var(run[k]), cs.var(next));
                    cur = next++;
                }
                last = cur;
                have_last = true;
                run.clear();
            }
            a[last] = minus_one;  // (1 - must_be_false - a) a = 0
        }
        a[next] = minus_one;
        cs.enforce(a, cs.var(next), cs.zero());
        bits_be.push_back(next++);
    }
    LC sum = cs.zero();
    Fe<P> coeff = fe_one<P>();
    for (size_t k = bits_be.size(); k-- > 0;) {
        sum[bits_be[k]] = coeff;
        coeff = fe_add<P>(coeff, coeff);
    }
    cs.enforce(sum, cs.var(cs.one()), cs.var(0));  // unpacking
    return cs.out;
}

}  // namespace lurk
