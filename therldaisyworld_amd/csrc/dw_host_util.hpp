// dw_host_util.hpp — host-side helpers of the C ABI that carry no HIP types, so that the CPU test suite can
// compile and exercise them with g++ (tests/test_abi_and_host.py).
#pragma once
#include <cstddef>
#include <initializer_list>

namespace dw {

// One allocation and its size, owned: released by the destructor or reset().  `Policy` provides
// `static int alloc(void**, size_t)` and `static int release(void*)`, both 0 on success.  Invariant: an empty
// block holds 0 bytes.
template <class Policy>
class Block {
public:
    Block() = default;
    Block(const Block&) = delete;
    Block& operator=(const Block&) = delete;
    Block(Block&& o) noexcept : p_(o.p_), bytes_(o.bytes_) { o.p_ = nullptr; o.bytes_ = 0; }
    Block& operator=(Block&& o) noexcept {
        if (this != &o) {
            reset();
            p_ = o.p_; bytes_ = o.bytes_;
            o.p_ = nullptr; o.bytes_ = 0;
        }
        return *this;
    }
    ~Block() { reset(); }

    void* raw() const { return p_; }
    size_t bytes() const { return bytes_; }
    void reset() {
        if (p_) (void)Policy::release(p_);
        p_ = nullptr;
        bytes_ = 0;
    }
    // At least `need` bytes.  A block that has to grow is replaced (its contents are not kept): by exactly `need`
    // bytes when `first_size` is 0, otherwise by twice its old size, `first_size` for the first allocation, and
    // never less than `need`.  On failure the block is empty and the allocator's code is returned.
    int reserve(size_t need, size_t first_size = 0) {
        if (bytes_ >= need) return 0;
        size_t want = first_size == 0 ? need : (bytes_ ? 2 * bytes_ : first_size);
        if (want < need) want = need;
        return take(want);
    }
    // releases what the block holds, then allocates exactly `bytes`
    int take(size_t bytes) {
        reset();
        void* p = nullptr;
        const int rc = Policy::alloc(&p, bytes);
        if (rc != 0) return rc;
        p_ = p;
        bytes_ = bytes;
        return 0;
    }

private:
    void* p_ = nullptr;
    size_t bytes_ = 0;
};

// The same with a typed accessor, for the kernels and the launch code.
template <class T, class Policy>
class Buf : public Block<Policy> {
public:
    T* get() const { return static_cast<T*>(this->raw()); }
};

template <class Policy>
struct GroupItem {
    Block<Policy>& owner;
    size_t bytes;
};

// Buffers that are only ever used together (the two planes of an un-quantised state, the near-tie queues and
// their overflow list, the regions of a snapshot) are allocated ALL OR NOTHING.  A group whose every block already
// holds its size is left alone; otherwise every block is released and allocated again.  When one allocation fails,
// what was allocated is given back and every block of the group is empty: a later call sees "not allocated" and
// retries (or reports the failure again) instead of finding some of the buffers and launching a kernel on a null
// other one.  Returns 0 or the first failing code.
template <class Policy>
int alloc_group(std::initializer_list<GroupItem<Policy>> group) {
    bool held = true;
    for (const auto& g : group) held = held && g.owner.bytes() >= g.bytes;
    if (held) return 0;
    for (const auto& g : group) g.owner.reset();
    for (const auto& g : group) {
        if (const int rc = g.owner.take(g.bytes)) {
            for (const auto& r : group) r.owner.reset();
            return rc;
        }
    }
    return 0;
}

}  // namespace dw
