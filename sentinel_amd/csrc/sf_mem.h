// sf_mem.h — who owns device and pinned host memory (host code only; no HIP
// header, so tests/mem_check.cpp runs it on malloc under the sanitizers).
//
//   MemOps   the seam to the backend: sf_host.h plugs in hipMalloc /
//            hipFree / hipHostMalloc / hipHostFree, the host test malloc / free
//            with a counter that fails the k-th allocation.  Nothing else.
//   DevPool  owns every pointer it handed out; what is left is freed by clear()
//            and by the destructor.  The structs that kernels take by value keep
//            their raw pointers: the pool that owns them sits beside the struct.
//   GrowBuf  a grow-only buffer: after a failed reserve it is empty, so the next
//            call allocates again.
//   Layout   offsets of the pieces of one staging buffer, 256-byte aligned.
//   StagePlan  one batch's arrays, each declared once: its room in the staging
//            buffer, its copy and the device pointer the kernels get (host
//            form), or the caller's pointer in place (device form).
//
// The rule for a set of buffers that grow together (a Work set, the token /
// concurrency / degrade work sets, ...): the set's capacity or first-use flag
// is written only after every allocation of the set has succeeded; on any
// failure the set's pool is cleared and its struct reset, so capacity reads 0
// and the next call builds the set again.
#pragma once
#include <assert.h>
#include <stddef.h>

#include <vector>

namespace sf {

// an int-returning step of a host function: 0 goes on, anything else is returned
#define SF_TRY(expr)                          \
    do {                                      \
        const int _rc = (expr);               \
        if (_rc) return _rc;                  \
    } while (0)

struct MemOps {                               // alloc: 0, or the error code the caller returns
    int (*dev_alloc)(void** p, size_t bytes);
    void (*dev_free)(void* p);
    int (*host_alloc)(void** p, size_t bytes);
    void (*host_free)(void* p);
};

// hipMalloc(0) is not asked for: an empty table still has an address
inline size_t nz(size_t bytes) { return bytes ? bytes : 16; }
inline size_t min16(size_t bytes) { return bytes < 16 ? 16 : bytes; }

class DevPool {
public:
    explicit DevPool(const MemOps& ops) : ops_(&ops) {}
    DevPool(const DevPool&) = delete;
    DevPool& operator=(const DevPool&) = delete;
    ~DevPool() { clear(); }

    // exactly `bytes` of device (alloc) or pinned host (alloc_host) memory; *p is null on failure
    template <class T> int alloc(T** p, size_t bytes) { return take((void**)p, bytes, false); }
    template <class T> int alloc_host(T** p, size_t bytes) { return take((void**)p, bytes, true); }

    // frees one pointer of this pool and nulls it.  false: not this pool's (nothing freed, p unchanged)
    template <class T> bool release(T*& p) {
        if (!p) return true;
        for (size_t i = own_.size(); i-- > 0;) {
            if (own_[i].p != (const void*)p) continue;
            drop(own_[i]);
            own_.erase(own_.begin() + (ptrdiff_t)i);
            p = nullptr;
            return true;
        }
        return false;
    }
    template <class... T> void release_all(T*&... p) { (release(p), ...); }

    // takes over everything `from` owns (a replacement built in a scratch pool, now complete)
    void adopt(DevPool& from) {
        own_.insert(own_.end(), from.own_.begin(), from.own_.end());
        from.own_.clear();
    }
    void clear() {
        for (size_t i = own_.size(); i-- > 0;) drop(own_[i]);
        own_.clear();
    }
    size_t count() const { return own_.size(); }

private:
    struct Entry { void* p; bool host; };
    int take(void** p, size_t bytes, bool host) {
        *p = nullptr;
        own_.reserve(own_.size() + 1);        // (no throw between the allocation and its record)
        const int rc = host ? ops_->host_alloc(p, bytes) : ops_->dev_alloc(p, bytes);
        if (rc) { *p = nullptr; return rc; }
        own_.push_back(Entry{*p, host});
        return 0;
    }
    void drop(const Entry& x) { x.host ? ops_->host_free(x.p) : ops_->dev_free(x.p); }
    const MemOps* ops_;
    std::vector<Entry> own_;
};

struct GrowBuf {
    void* p = nullptr;
    size_t bytes = 0;
    // at least `need` bytes: no-op when they are there, else free, then exactly `need`
    int reserve(DevPool& pool, size_t need) {
        if (need <= bytes) return 0;
        pool.release(p);
        bytes = 0;
        SF_TRY(pool.alloc(&p, need));
        bytes = need;
        return 0;
    }
    char* at(size_t off) const { return (char*)p + off; }
};

struct Layout {
    static size_t align_up(size_t x) { return (x + 255) & ~(size_t)255; }
    size_t take(size_t bytes) { const size_t o = off_; off_ += align_up(bytes); return o; }
    size_t take_if(bool on, size_t bytes) { return on ? take(bytes) : off_; }   // off: no room, the offset is not used
    size_t size() const { return off_; }
private:
    size_t off_ = 0;
};

// The staging of one batch: every array is declared once, with the address of
// the pointer the kernels read.  A host-form array gets room in the staging
// buffer (Layout's offsets, in declaration order) and a copy; a device-form
// array is read or written in place: its pointer is the caller's, it takes no
// room and no copy.  The input and the result form are independent.  An
// inout array (result form) is copied both ways.  `on`
// false: the pointer is null, no room, no copy, in either form.
//   size()   the room to reserve (the site decides when its buffer may move)
//   bind()   every staged pointer = base + its offset
//   upload() / download()   the copies in declaration order through
//            copy(dst, src, bytes) -> int; pieces of 0 bytes are skipped, the
//            first error is returned
// The pieces sit in an inline array: a plan never allocates.
class StagePlan {
public:
    static constexpr int CAP = 48;
    StagePlan(bool host_in, bool host_out) : host_in_(host_in), host_out_(host_out) {}
    StagePlan(const StagePlan&) = delete;
    StagePlan& operator=(const StagePlan&) = delete;

    // an input array of `bytes` at src; room: what the kernels may read past it
    template <class T> void in(bool on, const T** dev, const void* src, size_t bytes, size_t room = 0) {
        if (!on) *dev = nullptr;
        else if (!host_in_) *dev = (const T*)src;
        else add(dev, set<const T>, room ? room : bytes, (void*)src, bytes, UP);
    }
    // a result array of `bytes`, copied back to dst when asked
    template <class T> void out(bool on, T** dev, void* dst, size_t bytes, bool copy_back = true) {
        if (!on) *dev = nullptr;
        else if (!host_out_) *dev = (T*)dst;
        else add(dev, set<T>, bytes, dst, bytes, copy_back ? DOWN : NONE);
    }
    // an array the kernels update in place (the result form): copied up, and back when asked
    template <class T> void inout(bool on, T** dev, void* host, size_t bytes) {
        if (!on) *dev = nullptr;
        else if (!host_out_) *dev = (T*)host;
        else add(dev, set<T>, bytes, host, bytes, BOTH);
    }
    // device-only room, in either form
    template <class T> void scratch(bool on, T** dev, size_t bytes) {
        if (!on) *dev = nullptr;
        else add(dev, set<T>, bytes, nullptr, 0, NONE);
    }
    template <class T> void scratch(T** dev, size_t bytes) { scratch(true, dev, bytes); }

    size_t size() const { return lay_.size(); }
    void bind(void* base) {
        base_ = (char*)base;
        for (int i = 0; i < n_; i++) e_[i].set(e_[i].slot, base_ + e_[i].off);
    }
    template <class F> int upload(F&& copy) const {
        for (int i = 0; i < n_; i++)
            if ((e_[i].dir == UP || e_[i].dir == BOTH) && e_[i].bytes) SF_TRY(copy((void*)(base_ + e_[i].off), (const void*)e_[i].host, e_[i].bytes));
        return 0;
    }
    template <class F> int download(F&& copy) const {
        for (int i = 0; i < n_; i++)
            if ((e_[i].dir == DOWN || e_[i].dir == BOTH) && e_[i].bytes) SF_TRY(copy(e_[i].host, (const void*)(base_ + e_[i].off), e_[i].bytes));
        return 0;
    }

private:
    enum Dir : unsigned char { NONE, UP, DOWN, BOTH };
    struct Piece { void* slot; void (*set)(void*, char*); size_t off; void* host; size_t bytes; Dir dir; };
    template <class T> static void set(void* slot, char* p) { *(T**)slot = (T*)p; }
    void add(void* slot, void (*st)(void*, char*), size_t room, void* host, size_t bytes, Dir dir) {
        assert(n_ < CAP);
        e_[n_++] = Piece{slot, st, lay_.take(room), host, bytes, dir};
    }
    bool host_in_, host_out_;
    Layout lay_;
    char* base_ = nullptr;
    int n_ = 0;
    Piece e_[CAP];
};

}  // namespace sf
