// C++ host-mirror test of KEYED moduli (include/h2r_chips.hpp: KeyTable, AssignedInteger::keyed): the reference's three RSA vectors
// (src/chip.rs:683-816) verified under three keys of one key table in ONE call -- is_valid = 1, 1, 0 -- with the results of the same
// call on KeyTable::expand's per-element moduli; a zero key and an index out of range get their statuses.
// TEST CODE.  Build: tests/cpp_build.py (tests/test_keyed_moduli.py).
#include <cstdio>
#include <fstream>
#include <sstream>
#include <string>
#include <vector>

#include "h2r_chips.hpp"

using namespace h2r_host;

#define REQUIRE(cond)                                                                  \
    do {                                                                               \
        if (!(cond)) { std::fprintf(stderr, "FAILED %s:%d: %s\n", __FILE__, __LINE__, #cond); return 1; } \
    } while (0)

struct Kat { std::string name; int is_valid; std::vector<uint64_t> n, sig, hashed; };

static std::vector<Kat> load(const char *path) {
    std::vector<Kat> out; std::ifstream f(path); std::string line;
    while (std::getline(f, line)) {
        if (line.empty() || line[0] == '#') continue;
        std::istringstream is(line); Kat k; is >> k.name >> k.is_valid;
        auto rd = [&](std::vector<uint64_t> &v, int n) { for (int i = 0; i < n; ++i) { std::string h; is >> h; v.push_back(std::stoull(h, nullptr, 16)); } };
        rd(k.n, 32); rd(k.sig, 32); rd(k.hashed, 4);
        out.push_back(k);
    }
    return out;
}

int main(int argc, char **argv) {
    REQUIRE(argc == 2);
    std::vector<Kat> kats = load(argv[1]);
    REQUIRE(kats.size() == 3);
    RSAChip rsa_chip(2048, 5);
    const BigIntChip &chip = rsa_chip.bigint_chip();
    // keys: [KAT2's, zero, KAT3's, KAT1's]; elements 0..2 = the vectors, 3 names the zero key, 4 an index out of range
    std::vector<uint64_t> keys, sigs, hashed;
    const int order[4] = {1, -1, 2, 0};
    for (int k : order) { if (k < 0) keys.insert(keys.end(), 32, 0); else keys.insert(keys.end(), kats[k].n.begin(), kats[k].n.end()); }
    const std::vector<uint32_t> idx = {3, 0, 2, 1, 4};
    const size_t B = idx.size();
    for (size_t i = 0; i < B; ++i) {
        const Kat &k = kats[i < 3 ? i : 0];
        sigs.insert(sigs.end(), k.sig.begin(), k.sig.end()); hashed.insert(hashed.end(), k.hashed.begin(), k.hashed.end());
    }
    KeyTable table(chip, UnassignedInteger::from(keys, 4, 32));
    REQUIRE((table.status() == std::vector<uint8_t>{H2R_OK, H2R_E_ZERO_MODULUS, H2R_OK, H2R_OK}));
    AssignedRSASignature sign = rsa_chip.assign_signature(RSASignature{UnassignedInteger::from(sigs, B, 32)});
    AssignedInteger hm = chip.assign_integer(UnassignedInteger::from(hashed, B, 4));
    AssignedRSAPublicKey pk{table.select(idx), std::get<RSAPubE::Fix>(RSAPubE::fix(65537).v)};
    REQUIRE(pk.n.is_keyed() && BigIntChip::flags(pk.n, B) == H2R_F_KEYED_MODULI);
    VerifyResult res = rsa_chip.verify_pkcs1v15_signature(pk, hm, sign);
    AssignedRSAPublicKey pk_elem{table.expand(pk.n), std::get<RSAPubE::Fix>(pk.e)};
    REQUIRE(!pk_elem.n.is_keyed());
    VerifyResult ref = rsa_chip.verify_pkcs1v15_signature(pk_elem, hm, sign);
    const std::vector<uint8_t> want_status = {H2R_OK, H2R_OK, H2R_OK, H2R_E_ZERO_MODULUS, H2R_E_SHAPE};
    REQUIRE(res.status == want_status);
    REQUIRE((res.is_valid == std::vector<uint8_t>{1, 1, 0, 0, 0}));
    REQUIRE(ref.status[3] == H2R_E_ZERO_MODULUS && ref.status[4] == H2R_E_ZERO_MODULUS);   // (expand: zero for an index out of range)
    const std::vector<uint64_t> pk_limbs = res.powed.limbs(), pr_limbs = ref.powed.limbs();
    for (size_t i = 0; i < 3; ++i) {
        REQUIRE(ref.status[i] == H2R_OK && ref.is_valid[i] == res.is_valid[i]);
        for (size_t l = 0; l < 32; ++l) REQUIRE(pk_limbs[i * 32 + l] == pr_limbs[i * 32 + l]);
        std::vector<uint8_t> a(res.layout.elem_stride), b(res.layout.elem_stride), fa(res.layout.stream_bytes), fb(res.layout.stream_bytes);
        res.trace.download(a.data(), a.size(), i * res.layout.elem_stride);
        ref.trace.download(b.data(), b.size(), i * ref.layout.elem_stride);
        REQUIRE(h2r_verify_trace_flatten(chip.ctx(), &res.layout, a.data(), fa.data()) == H2R_OK);
        REQUIRE(h2r_verify_trace_flatten(chip.ctx(), &ref.layout, b.data(), fb.data()) == H2R_OK);
        REQUIRE(fa == fb);
    }
    // the BigIntChip forms take keyed moduli as `n` too
    AssignedInteger x = chip.assign_integer(UnassignedInteger::from(sigs, B, 32));
    BatchResult sq = chip.square_mod(x, pk.n), sq_ref = chip.square_mod(x, pk_elem.n);
    REQUIRE(sq.status == want_status);
    const std::vector<uint64_t> s1 = sq.value.limbs(), s2 = sq_ref.value.limbs();
    for (size_t i = 0; i < 3 * 32; ++i) REQUIRE(s1[i] == s2[i]);
    for (size_t i = 0; i < 3; ++i) REQUIRE(sq.trace.flatten(i) == sq_ref.trace.flatten(i));
    std::printf("CPP_KEYED_MIRROR_OK %zu\n", B);
    return 0;
}
