// ledger_check.cpp -- the ownership and the byte ledgers of the device buffer (csrc/devbuf.h) on a stand-in allocator, without
// a device: built with -fsanitize=address,undefined and run by `make ledger-check`.  A buffer inside a context-shaped struct --
// a direct member, one of a nested struct, of a base class, of an array -- lands in that context's ledger and in no other,
// with two contexts alive at once and with one built on a second thread; a buffer outside lands in none; a failed grow leaves
// the buffer as it was; and once everything is destroyed the ledgers, the process total and the allocator are back at zero
// (the sanitizer's leak check sees a buffer nobody freed).
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <thread>

#include "devbuf.h"

static int failures = 0;
#define CHECK(cond)                                                     \
  do {                                                                  \
    if (!(cond)) {                                                      \
      fprintf(stderr, "%s:%d: CHECK(%s) failed\n", __FILE__, __LINE__, #cond); \
      failures++;                                                       \
    }                                                                   \
  } while (0)

struct FakeMem {
  using error = int;
  using stream = void *;
  static constexpr int ok = 0;
  static inline std::atomic<long long> live{0}; // allocations not yet freed
  static inline std::atomic<int> fail_alloc{0}, fail_copy{0};
  static int alloc(void **q, size_t bytes)
  {
    if (fail_alloc) return 2;
    *q = malloc(bytes);
    live++;
    return *q ? 0 : 2;
  }
  static void free(void *p)
  {
    ::free(p);
    live--;
  }
  static int copy(void *dst, const void *src, size_t bytes, void *)
  {
    if (fail_copy) return 1;
    memcpy(dst, src, bytes);
    return 0;
  }
};
template <typename T> using Buf = MdpBuf<T, FakeMem>;

// shaped as mdp_ctx is: the ledger, the scope that opens it, members of every kind, the scope that closes it
struct Binning {
  Buf<unsigned> key_a, key_b;
  Buf<char> tmp;
};
struct Measure {
  bool on = false;
};
struct Rdf : Measure {
  int nbin = 0;
  Buf<int> tab;
  Binning bin;
};
struct Stage {
  Buf<double> st, part;
};
struct Spring : Stage {
  Buf<int> count;
};
struct Domain {
  Buf<double> sbuf, rbuf;
  Buf<int> lists[3];
};
struct Ctx {
  MdpLedger ledger;
  MdpLedgerScope ledger_open{&ledger};
  int device = 0;
  Buf<double> x;
  Buf<int> ring[4];
  Rdf rdf;
  Spring spring;
  Domain dd;
  Buf<char> last;
  MdpLedgerScope ledger_close{nullptr};

  // reserves something in every buffer; returns the bytes
  long long fill(size_t n)
  {
    Buf<double> *d[] = {&x, &spring.st, &spring.part, &dd.sbuf, &dd.rbuf};
    Buf<int> *i[] = {&ring[0], &ring[1], &ring[2], &ring[3], &rdf.tab, &spring.count, &dd.lists[0], &dd.lists[1], &dd.lists[2]};
    Buf<unsigned> *u[] = {&rdf.bin.key_a, &rdf.bin.key_b};
    Buf<char> *c[] = {&rdf.bin.tmp, &last};
    long long sum = 0;
    auto take = [&](auto *b, size_t m) {
      CHECK(b->reserve(m) == 0);
      sum += (long long) b->bytes();
    };
    for (auto *b : d) take(b, n);
    for (auto *b : i) take(b, n + 1);
    for (auto *b : u) take(b, n + 2);
    for (auto *b : c) take(b, n + 3);
    return sum;
  }
  bool all_mine() const
  {
    const MdpLedger *l = &ledger;
    bool ok = x.ledger == l && last.ledger == l && rdf.tab.ledger == l && rdf.bin.key_a.ledger == l && rdf.bin.key_b.ledger == l &&
              rdf.bin.tmp.ledger == l && spring.st.ledger == l && spring.part.ledger == l && spring.count.ledger == l &&
              dd.sbuf.ledger == l && dd.rbuf.ledger == l;
    for (const auto &b : ring) ok = ok && b.ledger == l;
    for (const auto &b : dd.lists) ok = ok && b.ledger == l;
    return ok;
  }
};

int main()
{
  auto &total = mdp_device_bytes_counter();
  CHECK(total == 0 && mdp_ledger_under_construction() == nullptr);
  {
    Buf<double> outside; // before any context
    CHECK(outside.ledger == nullptr);
    Ctx *a = new Ctx();
    CHECK(mdp_ledger_under_construction() == nullptr); // closed behind the last member
    Ctx *b = new Ctx();
    Buf<int> between; // behind two contexts
    CHECK(between.ledger == nullptr);
    Ctx *t = nullptr; // built on a second thread, used and destroyed on this one
    std::thread([&] {
      CHECK(mdp_ledger_under_construction() == nullptr);
      t = new Ctx();
      CHECK(mdp_ledger_under_construction() == nullptr);
    }).join();
    CHECK(a->all_mine() && b->all_mine() && t->all_mine());
    CHECK(a->ledger.bytes == 0 && b->ledger.bytes == 0 && t->ledger.bytes == 0 && total == 0);

    const long long na = a->fill(100), nb = b->fill(7), nt = t->fill(1000);
    CHECK(outside.reserve(50) == 0 && between.reserve(9) == 0);
    const long long nout = (long long) (outside.bytes() + between.bytes());
    CHECK(na > 0 && a->ledger.bytes == na);
    CHECK(nb > 0 && b->ledger.bytes == nb);
    CHECK(nt > 0 && t->ledger.bytes == nt);
    CHECK(total == na + nb + nt + nout); // the parts sum to the whole

    // growing keeps the contents and counts the difference; a reserve that fits changes nothing
    for (int k = 0; k < 100; k++) a->x.p[k] = k;
    const long long before = (long long) a->x.bytes();
    CHECK(a->x.reserve(100) == 0 && (long long) a->x.bytes() == before);
    CHECK(a->x.reserve(5000, true) == 0 && a->x.p[99] == 99.0);
    CHECK(a->ledger.bytes == na - before + (long long) a->x.bytes());
    // a grow that fails -- in the allocation, in the copy -- frees what it took and leaves the buffer as it was
    const long long held = a->ledger.bytes, tot = total, live = FakeMem::live;
    double *const p = a->x.p;
    const size_t cap = a->x.cap;
    FakeMem::fail_alloc = 1;
    CHECK(a->x.reserve(100000, true) == 2);
    FakeMem::fail_alloc = 0;
    FakeMem::fail_copy = 1;
    CHECK(a->x.reserve(100000, true) == 1);
    FakeMem::fail_copy = 0;
    CHECK(a->x.p == p && a->x.cap == cap && a->x.p[99] == 99.0);
    CHECK(a->ledger.bytes == held && total == tot && FakeMem::live == live);

    // swapping two buffers of one context exchanges the memory and leaves the ledger alone
    int *const p0 = a->ring[0].p;
    CHECK(a->dd.lists[1].reserve(3000) == 0);
    const long long held2 = a->ledger.bytes;
    const size_t c0 = a->ring[0].cap, c1 = a->dd.lists[1].cap;
    a->ring[0].swap(a->dd.lists[1]);
    CHECK(a->dd.lists[1].p == p0 && a->dd.lists[1].cap == c0 && a->ring[0].cap == c1 && a->ledger.bytes == held2);

    // an early release takes its bytes out of its own ledger alone
    const long long rb = (long long) b->rdf.bin.key_a.bytes();
    b->rdf.bin.key_a.release();
    CHECK(b->ledger.bytes == nb - rb && b->rdf.bin.key_a.p == nullptr && a->ledger.bytes == held2 && t->ledger.bytes == nt);

    // destruction gives everything back: the others' ledgers stand, the total falls by the context's
    const long long tot2 = total;
    delete a;
    CHECK(total == tot2 - held2 && b->ledger.bytes == nb - rb && t->ledger.bytes == nt);
    delete t;
    delete b;
    CHECK(total == nout);
  }
  CHECK(total == 0 && FakeMem::live == 0);
  if (failures) {
    fprintf(stderr, "ledger_check: %d checks failed\n", failures);
    return 1;
  }
  printf("ledger_check: ok\n");
  return 0;
}
