// bn254_capi_owners.h -- who owns what of the HIP runtime in the host code of the C ABI (bn254_capi*.hip): device buffers, pinned host buffers, streams and events as
// move-only members whose destructors release them, and the ring of pinned pieces the host-buffer entries stage their input through.  Included by
// bn254_capi_internal.h (which declares set_err and HIPCK before it); private like that header.  A struct made of these needs no free function: whoever destroys it
// (bn254_groth16_vk_free, bn254_plonk_vk_free, the last holder of a key set) makes the owning device current and waits for it first.
#pragma once

// A kernel launch that failed: no code object for this GPU means the library cannot run here at all (BN254_E_NO_DEVICE), everything else is the runtime's error.
// what: the launch, "kernel launch (what): ..."; nullptr: "kernel launch: ..."
static inline int launch_err(hipError_t e, const char* what) {
  return set_err(e == hipErrorNoBinaryForGpu || e == hipErrorInvalidDeviceFunction ? BN254_E_NO_DEVICE : BN254_E_HIP,
                 (what ? std::string("kernel launch (") + what + "): " : std::string("kernel launch: ")) + hipGetErrorString(e));
}

// Device memory for `cap()` elements.  ensure(n) is the one way it grows: a no-op while it holds n elements; otherwise the old memory is released FIRST -- hipFree waits
// for the device, so no batch is still using it -- and forgotten before anything is allocated: if the allocation fails the buffer is empty (null, capacity 0), never a
// stale pointer that a later call or the destructor would free a second time.  oom: the code for hipErrorOutOfMemory (the key sets answer BN254_E_NOMEM)
template <class T> class DevBuf {
 public:
  DevBuf() = default;
  DevBuf(DevBuf&& o) noexcept : p_(o.p_), cap_(o.cap_) { o.p_ = nullptr; o.cap_ = 0; }
  DevBuf& operator=(DevBuf&& o) noexcept { if (this != &o) { release(); p_ = o.p_; cap_ = o.cap_; o.p_ = nullptr; o.cap_ = 0; } return *this; }
  ~DevBuf() { release(); }
  int ensure(size_t n, int oom = BN254_E_HIP) {
    if (p_ && n <= cap_) return BN254_OK;
    release();
    const hipError_t e = hipMalloc((void**)&p_, (n ? n : 1) * sizeof(T));
    if (e != hipSuccess) { p_ = nullptr; return set_err(e == hipErrorOutOfMemory ? oom : BN254_E_HIP, std::string("hipMalloc: ") + hipGetErrorString(e)); }
    cap_ = n;
    return BN254_OK;
  }
  void release() { if (p_) (void)hipFree(p_); p_ = nullptr; cap_ = 0; }
  operator T*() const { return p_; }
  size_t cap() const { return cap_; }

 private:
  T* p_ = nullptr; size_t cap_ = 0;
};
// the same for pinned host memory
template <class T> class PinBuf {
 public:
  PinBuf() = default;
  PinBuf(PinBuf&& o) noexcept : p_(o.p_), cap_(o.cap_) { o.p_ = nullptr; o.cap_ = 0; }
  PinBuf& operator=(PinBuf&& o) noexcept { if (this != &o) { release(); p_ = o.p_; cap_ = o.cap_; o.p_ = nullptr; o.cap_ = 0; } return *this; }
  ~PinBuf() { release(); }
  int ensure(size_t n) {
    if (p_ && n <= cap_) return BN254_OK;
    release();
    const hipError_t e = hipHostMalloc((void**)&p_, (n ? n : 1) * sizeof(T), hipHostMallocDefault);
    if (e != hipSuccess) { p_ = nullptr; return set_err(BN254_E_HIP, std::string("hipHostMalloc: ") + hipGetErrorString(e)); }
    cap_ = n;
    return BN254_OK;
  }
  void release() { if (p_) (void)hipHostFree(p_); p_ = nullptr; cap_ = 0; }
  operator T*() const { return p_; }
  size_t cap() const { return cap_; }

 private:
  T* p_ = nullptr; size_t cap_ = 0;
};

// A non-blocking stream / an event, created by the first ensure() and not before: every stream of a process shares the runtime's few hardware queues, so none exists
// that is not used (DevState::aux has the measurement).  Events are created without timing unless ensure_timed() makes them.
class Stream {
 public:
  Stream() = default;
  Stream(Stream&& o) noexcept : s_(o.s_) { o.s_ = nullptr; }
  Stream& operator=(Stream&& o) noexcept { if (this != &o) { release(); s_ = o.s_; o.s_ = nullptr; } return *this; }
  ~Stream() { release(); }
  int ensure() { if (!s_) HIPCK(hipStreamCreateWithFlags(&s_, hipStreamNonBlocking)); return BN254_OK; }
  operator hipStream_t() const { return s_; }

 private:
  void release() { if (s_) (void)hipStreamDestroy(s_); s_ = nullptr; }
  hipStream_t s_ = nullptr;
};
class Event {
 public:
  Event() = default;
  Event(Event&& o) noexcept : ev_(o.ev_) { o.ev_ = nullptr; }
  Event& operator=(Event&& o) noexcept { if (this != &o) { release(); ev_ = o.ev_; o.ev_ = nullptr; } return *this; }
  ~Event() { release(); }
  int ensure() { if (!ev_) HIPCK(hipEventCreateWithFlags(&ev_, hipEventDisableTiming)); return BN254_OK; }
  int ensure_timed() { if (!ev_) HIPCK(hipEventCreate(&ev_)); return BN254_OK; }
  operator hipEvent_t() const { return ev_; }

 private:
  void release() { if (ev_) (void)hipEventDestroy(ev_); ev_ = nullptr; }
  hipEvent_t ev_ = nullptr;
};

// Host buffers.  The caller's memory is pageable, and a hipMemcpyAsync from pageable memory is neither asynchronous nor fast (the runtime stages it through its own
// bounce buffer while the calling thread waits).  So a host-buffer entry keeps a ring of three PINNED pieces: host threads copy piece i + 1 of the caller's buffers into
// the ring while piece i travels to the device (a true asynchronous copy on the copy stream) and the compute stream works; the compute stream waits, on the GPU, for
// last(), the event of the newest piece.  Only stream-scoped synchronisation.  Its owner's lock is held for the whole call: the ring belongs to one batch at a time.
#define HOST_RING 3
struct PinRing {
  Stream compute, copy;                 // the batch's kernels / its host-to-device copies
  // the three pieces are sized together (piece() bytes each) or not at all; the streams and the events come with the first size
  int ensure(size_t piece_bytes) {
    int rc;
    if ((rc = compute.ensure()) || (rc = copy.ensure())) return rc;
    if (piece_bytes <= piece_) return BN254_OK;
    piece_ = 0;
    for (auto& p : pin_) p.release();
    for (int i = 0; i < HOST_RING; i++)
      if ((rc = pin_[i].ensure(piece_bytes)) || (rc = ev_[i].ensure())) { for (auto& p : pin_) p.release(); return rc; }
    piece_ = piece_bytes;
    return BN254_OK;
  }
  size_t piece() const { return piece_; }
  void begin() { uses_ = 0; last_ = nullptr; }       // a new batch: every piece of the previous one has left (its call waited for the compute stream)
  // the next piece, free to be written: waits (on the host) until the piece that used its slot before has left for the device
  int acquire(uint8_t** pin) {
    const int slot = (int)(uses_ % HOST_RING);
    if (uses_ >= HOST_RING) HIPCK(hipEventSynchronize(ev_[slot]));
    *pin = pin_[slot];
    return BN254_OK;
  }
  // the copies of the acquired piece have been enqueued on the copy stream
  int commit() {
    const int slot = (int)(uses_ % HOST_RING);
    HIPCK(hipEventRecord(ev_[slot], copy));
    last_ = ev_[slot];
    uses_++;
    return BN254_OK;
  }
  // bytes [0, len) of a device buffer through the ring, fill(pin, from, k) writing bytes [from, from + k) into the pinned piece
  int push(uint8_t* dst, size_t len, const std::function<void(uint8_t*, size_t, size_t)>& fill) {
    for (size_t from = 0; from < len;) {
      const size_t k = len - from < piece_ ? len - from : piece_;
      uint8_t* pin;
      int rc = acquire(&pin);
      if (rc) return rc;
      fill(pin, from, k);
      HIPCK(hipMemcpyAsync(dst + from, pin, k, hipMemcpyHostToDevice, copy));
      if ((rc = commit())) return rc;
      from += k;
    }
    return BN254_OK;
  }
  hipEvent_t last() const { return last_; }           // of the newest piece (nullptr: none since begin())
  // a call that fails while pieces or earlier chunks may still be in flight: the ring and the staging buffers must be quiescent when the lock is released; the
  // error text of the failure is the one the caller reads
  int drain(int rc) {
    const std::string keep = g_err;
    (void)hipStreamSynchronize(copy); (void)hipStreamSynchronize(compute);
    g_err = keep;
    return rc;
  }

 private:
  PinBuf<uint8_t> pin_[HOST_RING]; Event ev_[HOST_RING]; size_t piece_ = 0, uses_ = 0; hipEvent_t last_ = nullptr;
};
