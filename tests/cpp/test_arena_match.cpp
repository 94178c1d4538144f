// Stand-alone host test of the trace arena's slot match (halo2_rsa_amd/csrc/h2r_arena_match.hpp): which record launches may leave
// the constant planes of their records alone.  No device, no library: g++ -std=c++17 -fsanitize=address,undefined.
#include <cstdio>
#include <cstdlib>

#include "h2r_arena_match.hpp"

using namespace h2r_arena_match;

static int g_fail = 0;
#define REQUIRE(x) do { if (!(x)) { std::printf("FAILED %s:%d: %s\n", __FILE__, __LINE__, #x); ++g_fail; } } while (0)

int main() {
    // RSA-2048, e = 65537: 19 records of 65,024 bytes from offset 5,120 of a 4,865 x 256-byte element; an arena of 1,024 elements
    Region r;
    r.device = 0; r.limb_width = 64; r.num_limbs = 32;
    r.base = 0x7f0000000000ull; r.elem_stride = 4865ull * 256; r.first_record_off = 5120; r.records_per_elem = 19; r.batch = 1024;
    r.bytes = r.batch * r.elem_stride;
    int owner_a = 0, owner_b = 0;
    r.owner = &owner_a;
    Registry reg;
    reg.add(r);
    Region r2 = r;
    r2.base = 0x7e0000000000ull; r2.owner = &owner_b;
    reg.add(r2);
    REQUIRE(reg.size() == 2);

    Launch l;
    l.device = 0; l.limb_width = 64; l.num_limbs = 32;
    l.trace = r.base; l.elem_stride = r.elem_stride; l.off_records = 5120; l.t_lo = 0; l.T = 19; l.elems = 1024;
    REQUIRE(reg.match(l));                                           // the whole region from its base
    { Launch m = l; m.trace = r2.base; REQUIRE(reg.match(m)); }      // the other region
    { Launch m = l; m.trace += 5 * r.elem_stride; m.elems = 1019; REQUIRE(reg.match(m)); }   // an element offset, up to the end
    { Launch m = l; m.trace += 5 * r.elem_stride; m.elems = 7; REQUIRE(reg.match(m)); }
    { Launch m = l; m.trace += 1023 * r.elem_stride; m.elems = 1; REQUIRE(reg.match(m)); }   // the last element
    { Launch m = l; m.trace += 1; REQUIRE(!reg.match(m)); }          // one byte off
    { Launch m = l; m.trace -= 1; REQUIRE(!reg.match(m)); }          // ... either way
    { Launch m = l; m.trace += 256; m.elems = 1; REQUIRE(!reg.match(m)); }                   // not a whole number of elements
    { Launch m = l; m.elem_stride += 256; REQUIRE(!reg.match(m)); }  // wrong stride
    { Launch m = l; m.elem_stride = 0; REQUIRE(!reg.match(m)); }
    { Launch m = l; m.off_records = 0; REQUIRE(!reg.match(m)); }     // another records offset
    { Launch m = l; m.T = 20; REQUIRE(!reg.match(m)); }              // T beyond records_per_elem
    { Launch m = l; m.t_lo = 10; m.T = 9; REQUIRE(reg.match(m)); }   // a segment of the exponent: records [10, 19)
    { Launch m = l; m.t_lo = 10; m.T = 10; REQUIRE(!reg.match(m)); }
    { Launch m = l; m.t_lo = 0xffffffffu; m.T = 2; REQUIRE(!reg.match(m)); }                 // (no 32-bit wrap)
    { Launch m = l; m.elems = 1025; REQUIRE(!reg.match(m)); }        // past the region's end
    { Launch m = l; m.trace += 5 * r.elem_stride; m.elems = 1020; REQUIRE(!reg.match(m)); }
    { Launch m = l; m.trace += 1024 * r.elem_stride; m.elems = 1; REQUIRE(!reg.match(m)); }  // the first byte behind the region
    { Launch m = l; m.elems = ~0ull; REQUIRE(!reg.match(m)); }       // (no 64-bit wrap)
    { Launch m = l; m.elems = 0; REQUIRE(!reg.match(m)); }
    { Launch m = l; m.T = 0; REQUIRE(!reg.match(m)); }
    { Launch m = l; m.device = 1; REQUIRE(!reg.match(m)); }          // another device
    { Launch m = l; m.num_limbs = 16; REQUIRE(!reg.match(m)); }      // another shape
    { Launch m = l; m.limb_width = 32; REQUIRE(!reg.match(m)); }
    { Launch m = l; m.trace = 0x100000; REQUIRE(!reg.match(m)); }    // a plain buffer
    { Launch m = l; m.trace = 0; REQUIRE(!reg.match(m)); }

    reg.unregister_owner(&owner_a);                                  // a region unregistered: its addresses match nothing any more
    REQUIRE(reg.size() == 1);
    REQUIRE(!reg.match(l));
    { Launch m = l; m.trace = r2.base; REQUIRE(reg.match(m)); }
    reg.unregister_owner(&owner_a);                                  // (twice is harmless)
    reg.unregister_owner(&owner_b);
    REQUIRE(reg.size() == 0);
    { Launch m = l; m.trace = r2.base; REQUIRE(!reg.match(m)); }

    if (g_fail) { std::printf("ARENA_MATCH_FAILED %d\n", g_fail); return 1; }
    std::printf("ARENA_MATCH_OK\n");
    return 0;
}
