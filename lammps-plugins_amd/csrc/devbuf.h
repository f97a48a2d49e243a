// devbuf.h -- the library's device buffer and the byte ledgers it keeps.  Nothing here names HIP: the allocate / free /
// copy triple comes in as the policy M (MdpHipMem in mdp_common.h; a stand-in in tests/native/ledger_check.cpp).
#pragma once

#include <atomic>
#include <cstddef>

// bytes of device memory currently held by the library's buffers in this process (memory_usage(), pair_rebomos.cpp:1113-1124)
inline std::atomic<long long> &mdp_device_bytes_counter()
{
  static std::atomic<long long> bytes{0}; // several contexts (threads) allocate concurrently
  return bytes;
}

// ... and by the buffers of ONE context: mdp_ctx holds a ledger, and every buffer inside it, at any depth, finds it
// without being told.  Default member initialisers run in declaration order, so between the MdpLedgerScope members that
// open and close mdp_ctx (`ledger_open`, `ledger_close`) the thread's "ledger under construction" is that context's, and
// a buffer's initialiser copies it.  A buffer made anywhere else gets none and counts in the process total alone.
struct MdpLedger {
  long long bytes = 0;
};
inline MdpLedger *&mdp_ledger_under_construction()
{
  static thread_local MdpLedger *l = nullptr;
  return l;
}
struct MdpLedgerScope {
  explicit MdpLedgerScope(MdpLedger *l) { mdp_ledger_under_construction() = l; }
};

// device buffer that only grows, and frees itself
template <typename T, class M> struct MdpBuf {
  T *p = nullptr;
  size_t cap = 0;
  MdpLedger *ledger = mdp_ledger_under_construction();
  MdpBuf() = default;
  MdpBuf(const MdpBuf &) = delete;
  MdpBuf &operator=(const MdpBuf &) = delete;
  ~MdpBuf() { release(); }
  typename M::error reserve(size_t n, bool keep = false, typename M::stream s = nullptr)
  {
    if (n <= cap) return M::ok;
    size_t ncap = n + n / 8 + 64;
    T *q = nullptr;
    typename M::error e = M::alloc((void **) &q, ncap * sizeof(T));
    if (e != M::ok) return e;
    if (keep && p && cap) {
      e = M::copy(q, p, cap * sizeof(T), s);
      if (e != M::ok) {
        M::free(q); // the buffer stays as it was
        return e;
      }
    }
    if (p) M::free(p);
    count((long long) ((ncap - cap) * sizeof(T)));
    p = q;
    cap = ncap;
    return M::ok;
  }
  void release()
  {
    if (p) M::free(p);
    count(-(long long) (cap * sizeof(T)));
    p = nullptr;
    cap = 0;
  }
  size_t bytes() const { return cap * sizeof(T); }
  // exchanges the memory of two buffers; each stays in its own ledger, so both must belong to the same one
  void swap(MdpBuf &o)
  {
    T *const q = p;
    p = o.p;
    o.p = q;
    const size_t c = cap;
    cap = o.cap;
    o.cap = c;
  }

private:
  void count(long long d)
  {
    mdp_device_bytes_counter() += d;
    if (ledger) ledger->bytes += d;
  }
};
