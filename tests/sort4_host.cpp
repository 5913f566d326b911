// sort4 (glaze_amd/csrc/device/sort4.h) as the host compiles it, against std::sort: every assignment of {three hit keys, the miss marker}
// to the four children, in both orders.  Built and run by tests/test_sort4_host.py; prints the number of assignments checked.
#include <algorithm>
#include <cstdint>
#include <cstdio>
#include <functional>

#include "device/sort4.h"

template <bool DESCENDING>
static int check(const uint32_t (&values)[4]) {
  int bad = 0;
  for (int n = 0; n < 256; ++n) {
    const uint32_t in[4] = {values[n & 3], values[(n >> 2) & 3], values[(n >> 4) & 3], values[(n >> 6) & 3]};
    uint32_t want[4] = {in[0], in[1], in[2], in[3]}, k[4] = {in[0], in[1], in[2], in[3]};
    if (DESCENDING) std::sort(want, want + 4, std::greater<uint32_t>()); else std::sort(want, want + 4);
    glz::sort4<DESCENDING>(k[0], k[1], k[2], k[3]);
    if (!std::equal(k, k + 4, want)) {
      ++bad;
      printf("%s %08x %08x %08x %08x -> %08x %08x %08x %08x, std::sort %08x %08x %08x %08x\n", DESCENDING ? "descending" : "ascending", in[0], in[1], in[2], in[3],
             k[0], k[1], k[2], k[3], want[0], want[1], want[2], want[3]);
    }
  }
  return bad;
}

int main() {
  // key = distance bits (the low ten cleared) | child << 8 (device/intersect.h box_key); two of the hits at the SAME distance, told apart
  // by their child bits alone.  Near first: a miss is 0xFFFFFFFF.  Far first (a pass of any-hit rays): bit 0 set, a miss is 0.
  const uint32_t near_first[4] = {0x3F800000u | 0x100u, 0x3F800000u | 0x200u, 0x40490C00u | 0x300u, 0xFFFFFFFFu};
  const uint32_t far_first[4] = {0x3F800000u | 0x000u | 1u, 0x3F800000u | 0x300u | 1u, 0x40490C00u | 0x100u | 1u, 0u};
  const int bad = check<false>(near_first) + check<true>(far_first) + check<false>(far_first) + check<true>(near_first);
  printf("%d assignments checked, %d wrong\n", 4 * 256, bad);
  return bad ? 1 : 0;
}
