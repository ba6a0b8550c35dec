// Host-only test of the structured trace LDE's planning and bookkeeping (zk-lisp_amd/csrc/
// lde_plan.h): which columns go to the column map, which to each period group, which slices are
// cleared, and what the book remembers from call to call.  Stand-alone (no device code), so it
// can be built with -fsanitize=address,undefined; tests/test_column_structure_lde.py does that.
#include <stdio.h>
#include <stdlib.h>

#include "../../zk-lisp_amd/csrc/lde_plan.h"

using namespace zkl;
using Runs = std::vector<std::pair<uint32_t, uint32_t>>;
using Cols = std::vector<uint32_t>;
constexpr uint32_t GEN = LDE_COL_GENERAL;

#define CHECK(x)                                                        \
  do {                                                                  \
    if (!(x)) {                                                         \
      fprintf(stderr, "%s:%d: check failed: %s\n", __FILE__, __LINE__, #x); \
      exit(1);                                                          \
    }                                                                   \
  } while (0)

static char bufs[4][16];  // stand-ins for device addresses (never dereferenced)

static LdePlan plan(ZeroBook& b, const Cols& per, size_t n, int coef = 0, int lde = 1) {
  const size_t N = 16 * n;
  b.begin(bufs[coef], bufs[lde], n, N, per.size());
  CHECK(b.coef == nullptr);  // invalid while a call queues its writes
  LdePlan pl = plan_structured_lde(per.data(), (uint32_t)per.size(), n, b);
  b.commit(bufs[coef], bufs[lde], n, N, per.size());
  return pl;
}

int main() {
  const size_t n = 1024;
  {  // all zero, then the same again: nothing left to clear
    ZeroBook b;
    LdePlan pl = plan(b, Cols(7, 0), n);
    CHECK(pl.general.empty() && pl.pcols.empty() && pl.nonzero.empty());
    CHECK((pl.clear_all == Runs{{0, 7}}) && pl.clear_tail.empty());
    CHECK(pl.zero == std::vector<uint8_t>(7, 1));
    pl = plan(b, Cols(7, 0), n);
    CHECK(pl.clear_all.empty() && pl.clear_tail.empty());
  }
  {  // none zero
    ZeroBook b;
    LdePlan pl = plan(b, Cols(5, GEN), n);
    CHECK((pl.general == Cols{0, 1, 2, 3, 4}) && (pl.nonzero == pl.general));
    CHECK(pl.clear_all.empty() && pl.clear_tail.empty() && pl.pcols.empty());
  }
  {  // alternating zero / general: every run has length 1, one map for all general columns
    ZeroBook b;
    LdePlan pl = plan(b, Cols{0, GEN, 0, GEN, 0, GEN, 0}, n);
    CHECK((pl.general == Cols{1, 3, 5}));
    CHECK((pl.clear_all == Runs{{0, 1}, {2, 3}, {4, 5}, {6, 7}}));
  }
  {  // first and last column of each class; periods grouped in ascending order
    ZeroBook b;
    LdePlan pl = plan(b, Cols{32, 0, GEN, 1, 128, GEN, 2, 0, 32}, n);
    CHECK((pl.general == Cols{2, 5}));
    CHECK((pl.pcols == Cols{3, 6, 0, 8, 4}) && (pl.pper == Cols{1, 2, 32, 32, 128}));
    CHECK((pl.nonzero == Cols{0, 2, 3, 4, 5, 6, 8}));
    CHECK((pl.clear_all == Runs{{1, 2}, {7, 8}}));
    CHECK((pl.clear_tail == Runs{{0, 1}, {3, 5}, {6, 7}, {8, 9}}));  // nothing known yet
    pl = plan(b, Cols{32, 0, GEN, 1, 128, GEN, 2, 0, 32}, n);
    CHECK(pl.clear_all.empty() && pl.clear_tail.empty());
  }
  {  // P = n, P > n, a period that is no power of two, a period above the limit: general
    ZeroBook b;
    LdePlan pl = plan(b, Cols{128, 64, 24, 256, 3}, 128);
    CHECK((pl.general == Cols{0, 2, 3, 4}) && (pl.pcols == Cols{1}));
    CHECK(pl.clear_tail.empty());  // n <= LDE_P_MAX: the head is the whole column
    pl = plan(b, Cols{128, 64}, 64);
    CHECK((pl.general == Cols{0, 1}) && pl.pcols.empty());
  }
  {  // one column through general -> 32 -> zero -> 2 -> general -> zero, a neighbour staying zero
    ZeroBook b;
    LdePlan pl = plan(b, Cols{GEN, 0}, n);
    CHECK((pl.clear_all == Runs{{1, 2}}));
    pl = plan(b, Cols{32, 0}, n);
    CHECK(pl.clear_all.empty() && (pl.clear_tail == Runs{{0, 1}}));  // the transform wrote the tail
    CHECK(b.known[0] == ZeroBook::TAIL && b.known[1] == ZeroBook::ZERO);
    pl = plan(b, Cols{0, 0}, n);
    CHECK((pl.clear_all == Runs{{0, 1}}) && pl.clear_tail.empty());  // head and lde are not zero
    pl = plan(b, Cols{2, 0}, n);
    CHECK(pl.clear_all.empty() && pl.clear_tail.empty());  // a zero column's tail is zero
    CHECK(b.known[0] == ZeroBook::TAIL);
    pl = plan(b, Cols{GEN, 0}, n);
    CHECK(b.known[0] == ZeroBook::UNKNOWN && pl.clear_all.empty());
    pl = plan(b, Cols{0, 0}, n);
    CHECK((pl.clear_all == Runs{{0, 1}}));
  }
  {  // another buffer, another shape, another width: everything forgotten
    ZeroBook b;
    plan(b, Cols(3, 0), n);
    CHECK(plan(b, Cols(3, 0), n).clear_all.empty());
    CHECK((plan(b, Cols(3, 0), n, 2, 1).clear_all == Runs{{0, 3}}));  // coef reallocated
    CHECK((plan(b, Cols(3, 0), n, 2, 3).clear_all == Runs{{0, 3}}));  // lde reallocated
    CHECK((plan(b, Cols(3, 0), 2 * n, 2, 3).clear_all == Runs{{0, 3}}));
    CHECK((plan(b, Cols(4, 0), 2 * n, 2, 3).clear_all == Runs{{0, 4}}));
    CHECK(plan(b, Cols(4, 0), 2 * n, 2, 3).clear_all.empty());
    b.all_unknown();  // a dense call (the host-trace upload, the switch off)
    CHECK((plan(b, Cols(4, 0), 2 * n, 2, 3).clear_all == Runs{{0, 4}}));
  }
  {  // writes by others: only those that reach a buffer forget the states
    ZeroBook b;
    static char arena[4096];
    const size_t sn = 4, sN = 8, sW = 2;  // coef: 2 * 4 * 16 = 128 bytes, lde: 256 bytes
    auto again = [&] {
      b.begin(arena + 1024, arena + 2048, sn, sN, sW);
      const uint32_t per[2] = {0, 0};
      LdePlan pl = plan_structured_lde(per, 2, sn, b);
      b.commit(arena + 1024, arena + 2048, sn, sN, sW);
      return pl.clear_all.size();
    };
    CHECK(again() == 1 && again() == 0);
    b.wrote(arena, 1024, 16);  // ends where coef begins
    CHECK(again() == 0);
    b.wrote(arena + 1024 + 128, 64, 16);  // just past coef
    CHECK(again() == 0);
    b.wrote(arena + 1024 + 127, 1, 16);  // its last byte
    CHECK(again() == 1 && again() == 0);
    b.wrote(arena + 2000, 64, 16);  // into lde
    CHECK(again() == 1 && again() == 0);
    b.wrote(arena + 2048 + 256, 0, 16);  // unknown length, above both
    CHECK(again() == 0);
    b.wrote(arena + 2048, 0, 16);  // unknown length at lde (a free)
    CHECK(again() == 1);
  }
  printf("lde_plan_test ok\n");
  return 0;
}
