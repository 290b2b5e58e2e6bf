// proof_assemble.hpp — what the synchronous prover (prover.hip) and the stream-ordered one (prove_async.hip) share: the fixed-base tables of a
// key's alpha_1, beta_1, delta_1, delta_2, the host's proof assembly, and the view of a resident key a zkg_prover handle is made from.
#pragma once
#include "common.hpp"
#include <vector>

struct zkg_crs;

namespace zk {

// Host-side fixed-base table of one key element P (alpha_1, beta_1, delta_1, delta_2): entry [j][d-1] = d * 16^j * P, affine.  k * P for a
// 254-bit k is then 64 mixed additions and no doubling (~20 us for G1) instead of 254 doublings + ~127 additions (~130 us): the products
// r*delta, s*delta, rs*delta, s*alpha, r*beta that every proof needs cost less than one variable-base multiplication together.
template <class F> struct CombTable {
    std::vector<zk::Affine<F>> t;               // 64 x 15
    void build(const zk::Affine<F> &base) {
        // all 960 multiples in XYZZ first, then ONE inversion for the lot (Montgomery's trick over their ZZZ): a to_affine per entry was
        // 960 Fermat inversions, 10 - 25 ms of every key load
        std::vector<zk::XYZZ<F>> p(64 * 15);
        zk::XYZZ<F> row = zk::XYZZ<F>::from_affine(base);                        // 16^j * P
        for (int j = 0; j < 64; ++j) {
            zk::XYZZ<F> cur = row;
            for (int d = 1; d <= 15; ++d) { p[j * 15 + d - 1] = cur; cur.add(row); }
            for (int k = 0; k < 4; ++k) row = row.dbl();
        }
        t.assign(64 * 15, zk::Affine<F>::inf());
        std::vector<F> pre(p.size());
        F run = F::one();
        for (size_t i = 0; i < p.size(); ++i) { pre[i] = run; if (!p[i].is_inf()) run = run * p[i].zzz; }
        F inv = run.inverse();
        for (size_t i = p.size(); i-- > 0;) {
            if (p[i].is_inf()) continue;
            F zi = inv * pre[i];                                                 // 1 / ZZZ_i
            inv = inv * p[i].zzz;
            F z1 = zi * p[i].zz, zi2 = z1.sqr();                                 // ZZ / ZZZ = 1 / Z;  1 / ZZ
            t[i] = zk::Affine<F>{p[i].x * zi2, p[i].y * zi};
        }
    }
    zk::XYZZ<F> mul(const uint32_t k[8]) const {                                  // canonical little-endian scalar
        zk::XYZZ<F> acc = zk::XYZZ<F>::inf();
        for (int j = 0; j < 64; ++j) { uint32_t d = (k[j >> 3] >> (4 * (j & 7))) & 15u; if (d) acc.madd(t[j * 15 + d - 1]); }
        return acc;
    }
};
static constexpr size_t COMB_ENTRIES = 64 * 15;

// the key's part of a proof's algebra: alpha_1 and beta_2 as points, the four tables for the products with r, s and r s
struct ProofKey {
    G1Affine alpha_g1; G2Affine beta_g2;
    const CombTable<Fq> *alpha1 = nullptr, *beta1 = nullptr, *delta1 = nullptr; const CombTable<Fq2> *delta2 = nullptr;
};
// proof bytes from the four multi-exponentiations' results (W1: A, B_1, L over the whole witness [1 | w]; prover.hip):
// A = alpha + r delta + W_a, B = beta + s delta_2 + W_b2, C = s alpha + r beta_1 + rs delta + s W_a + r W_b1 + L + H
void assemble_proof(const ProofKey &key, const Fr &r, const Fr &s, const G1 W1[3], const G2 &Wb2, const G1 &Ht, uint8_t *out);

// What a zkg_prover handle borrows from a resident key (prover.hip fills it in; every pointer stays the key's).
struct CrsProverView {
    uint32_t n = 0, l = 0, C = 0; size_t m = 0; int device = 0; bool h_sharded = false;
    const uint32_t *rp[3] = {nullptr, nullptr, nullptr}, *col[3] = {nullptr, nullptr, nullptr}; const uint64_t *val[3] = {nullptr, nullptr, nullptr}; size_t nnz[3] = {0, 0, 0};   // DEVICE: A, B, C by rows
    const WindowTable *H = nullptr; uint32_t h_row_merge = 1;
    const G1Affine *A_query = nullptr, *B_g1 = nullptr, *L_query = nullptr; const G2Affine *B_g2 = nullptr;   // DEVICE: n + 1, n + 1, n - l, n + 1 points
    ProofKey key;
};
void crs_prover_view(const zkg_crs *crs, CrsProverView &v);
// the key counts its live prover handles (zkg_crs_shard_h refuses while there is one).  +1 fails (false) on a key with H shards.
bool crs_prover_ref(zkg_crs *crs, int delta);

}  // namespace zk
