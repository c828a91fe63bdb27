// The resident-expansion registry (csrc/nf4_resident.h) on its own, with fake device pointers and a payload that
// counts its live instances: insert, hit, every kind of miss, the byte budget, drop and clear.  Built with
// -fsanitize=address,undefined by tests/test_nf4_resident_cpu.py; exits 0 when every check holds.
#include "nf4_resident.h"

#include <cstdio>
#include <cstdlib>
#include <memory>
#include <vector>

namespace {

int live = 0;

struct Payload {           // stands for the tensors an entry holds: heap memory with a counted lifetime
  std::shared_ptr<std::vector<int>> data;
  explicit Payload(int tag) : data(new std::vector<int>(64, tag), [](std::vector<int>* p) { --live; delete p; }) {
    ++live;
  }
  int tag() const { return (*data)[0]; }
};

#define CHECK(c)                                                   \
  do {                                                             \
    if (!(c)) {                                                    \
      std::fprintf(stderr, "%s:%d: CHECK(%s)\n", __FILE__, __LINE__, #c); \
      std::exit(1);                                                \
    }                                                              \
  } while (0)

Nf4ResidentKey key(uintptr_t codes, uintptr_t scales, int64_t n, int64_t k, uint64_t vc = 0, uint64_t vs = 0) {
  Nf4ResidentKey x;
  x.codes = codes, x.scales = scales, x.n = n, x.k = k, x.codes_version = vc, x.scales_version = vs;
  return x;
}

}  // namespace

int main() {
  const int64_t budget = 1000;
  {
    Nf4ResidentRegistry<Payload> r;
    // insert + hit
    CHECK(r.find(key(0x1000, 0x2000, 64, 64)) == nullptr);
    CHECK(r.insert(key(0x1000, 0x2000, 64, 64), 400, budget, Payload(1)) != nullptr);
    CHECK(r.bytes() == 400 && r.size() == 1 && live == 1);
    Payload* p = r.find(key(0x1000, 0x2000, 64, 64));
    CHECK(p && p->tag() == 1);
    CHECK(r.find(key(0x1000, 0x2000, 64, 64)) == p);          // a hit changes nothing
    CHECK(r.key_at(0x1000) && r.key_at(0x1000)->n == 64 && r.key_at(0x3000) == nullptr);

    // every field of the key: a mismatch is a miss AND drops the entry
    const Nf4ResidentKey wrong[] = {key(0x1000, 0x2001, 64, 64), key(0x1000, 0x2000, 128, 64),
                                    key(0x1000, 0x2000, 64, 128), key(0x1000, 0x2000, 64, 64, 1, 0),
                                    key(0x1000, 0x2000, 64, 64, 0, 1)};
    for (const auto& w : wrong) {
      CHECK(r.find(w) == nullptr);
      CHECK(r.size() == 0 && r.bytes() == 0 && live == 0);
      CHECK(r.find(key(0x1000, 0x2000, 64, 64)) == nullptr);  // the old key does not come back
      CHECK(r.insert(key(0x1000, 0x2000, 64, 64), 400, budget, Payload(1)) != nullptr);
    }
    // another pointer is another entry and leaves this one alone
    CHECK(r.find(key(0x5000, 0x2000, 64, 64)) == nullptr && r.size() == 1);

    // the re-expansion after a version miss replaces the entry
    CHECK(r.find(key(0x1000, 0x2000, 64, 64, 7, 0)) == nullptr);
    CHECK(r.insert(key(0x1000, 0x2000, 64, 64, 7, 0), 400, budget, Payload(2)) != nullptr);
    CHECK(r.find(key(0x1000, 0x2000, 64, 64, 7, 0))->tag() == 2 && r.bytes() == 400 && live == 1);

    // budget: exactly full is admitted, one byte more is not, and nothing is evicted for it
    CHECK(r.admits(600, budget) && !r.admits(601, budget));
    CHECK(r.insert(key(0x6000, 0x7000, 64, 64), 601, budget, Payload(3)) == nullptr);
    CHECK(r.size() == 1 && r.bytes() == 400 && live == 1);
    CHECK(r.insert(key(0x6000, 0x7000, 64, 64), 600, budget, Payload(3)) != nullptr);
    CHECK(r.bytes() == 1000 && r.size() == 2 && live == 2);
    CHECK(r.insert(key(0x8000, 0x9000, 64, 64), 1, budget, Payload(4)) == nullptr);
    CHECK(r.find(key(0x1000, 0x2000, 64, 64, 7, 0))->tag() == 2 && r.find(key(0x6000, 0x7000, 64, 64))->tag() == 3);
    // budgets that admit nothing; sizes that would overflow the sum
    CHECK(!r.admits(1, 0) && !r.admits(1, -5) && !r.admits(-1, budget) && !r.admits(INT64_MAX, budget));
    CHECK(!r.admits(INT64_MAX, INT64_MAX));                   // 1000 bytes already resident
    // a smaller budget later keeps what is there and admits nothing new
    CHECK(r.insert(key(0x8000, 0x9000, 64, 64), 1, 500, Payload(4)) == nullptr && r.size() == 2);

    // drop
    CHECK(r.drop(0x6000) && !r.drop(0x6000));
    CHECK(r.bytes() == 400 && r.size() == 1 && live == 1);
    CHECK(r.insert(key(0x8000, 0x9000, 64, 64), 600, budget, Payload(4)) != nullptr);

    // clear releases every payload; the registry is usable afterwards
    r.clear();
    CHECK(r.bytes() == 0 && r.size() == 0 && live == 0);
    CHECK(r.find(key(0x1000, 0x2000, 64, 64, 7, 0)) == nullptr);
    CHECK(r.insert(key(0x1000, 0x2000, 64, 64), 1000, budget, Payload(5)) != nullptr && live == 1);

    // many entries in and out
    r.clear();
    for (uintptr_t i = 0; i < 500; ++i) CHECK(r.insert(key(0x10000 + 64 * i, 1, 64, 64), 2, budget, Payload((int)i)));
    CHECK(r.bytes() == 1000 && live == 500 && !r.admits(1, budget));
    for (uintptr_t i = 0; i < 500; i += 2) CHECK(r.drop(0x10000 + 64 * i));
    CHECK(r.bytes() == 500 && live == 250);
    for (uintptr_t i = 1; i < 500; i += 2) CHECK(r.find(key(0x10000 + 64 * i, 1, 64, 64))->tag() == (int)i);
  }
  CHECK(live == 0);                                           // the destructor releases the rest
  std::puts("nf4_resident registry: ok");
  return 0;
}
