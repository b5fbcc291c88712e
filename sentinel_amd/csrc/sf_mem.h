// sf_mem.h — who owns device and pinned host memory (host code only; no HIP
// header, so tests/mem_check.cpp runs it on malloc under the sanitizers).
//
//   MemOps   the seam to the backend: sf_engine.cpp plugs in hipMalloc /
//            hipFree / hipHostMalloc / hipHostFree, the host test malloc / free
//            with a counter that fails the k-th allocation.  Nothing else.
//   DevPool  owns every pointer it handed out; what is left is freed by clear()
//            and by the destructor.  The structs that kernels take by value keep
//            their raw pointers: the pool that owns them sits beside the struct.
//   GrowBuf  a grow-only buffer: after a failed reserve it is empty, so the next
//            call allocates again.
//   Layout   offsets of the pieces of one staging buffer, 256-byte aligned.
//
// The rule for a set of buffers that grow together (a Work set, the token /
// concurrency / degrade work sets, ...): the set's capacity or first-use flag
// is written only after every allocation of the set has succeeded; on any
// failure the set's pool is cleared and its struct reset, so capacity reads 0
// and the next call builds the set again.
#pragma once
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

}  // namespace sf
