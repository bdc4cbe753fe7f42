// The owner of an engine's (or an env pool's) device and pinned allocations: every buffer is allocated into a pointer member — its
// slot — through one of these, and release_all() or the destructor frees whatever is live.  Plain C++17 over a backend, so that the
// bookkeeping is tested on the CPU against a counting fake (tests/host_mem_probe.cpp); frl_api.hip supplies the HIP one.
//
// Backend: error_t, ok, stream_t and five static functions —
//   error_t device_alloc(void**, size_t bytes);                  error_t device_free(void*);
//   error_t pinned_alloc(void**, size_t bytes, unsigned flags);  error_t pinned_free(void*);
//   error_t memset_async(void*, int value, size_t bytes, stream_t);
//
// A record is a slot, not a block: what is freed is the block the slot holds at that moment, so two slots of one kind may trade
// blocks (frl_rollout swaps obs and obs_next).  The owner keeps the slots' addresses: whatever holds them must not move.
#pragma once
#include <cassert>
#include <cstddef>
#include <vector>

namespace frl {

enum MemKind { MEM_DEVICE, MEM_PINNED };

template <class B>
class MemOwner {
public:
    using error_t = typename B::error_t;

    MemOwner() = default;
    MemOwner(const MemOwner&) = delete;
    MemOwner& operator=(const MemOwner&) = delete;
    ~MemOwner() { release_all(); }

    // count elements of T into *slot, which is null or holds a block of this owner (freed and forgotten first).
    // On failure the slot is null and no record remains; count == 0 succeeds, leaves the slot null and records nothing.
    template <class T>
    error_t alloc(T** slot, size_t count, MemKind kind, unsigned pinned_flags = 0) {
        release(slot);
        if (count == 0) return B::ok;
        void* p = nullptr;
        const error_t err = kind == MEM_DEVICE ? B::device_alloc(&p, count * sizeof(T)) : B::pinned_alloc(&p, count * sizeof(T), pinned_flags);
        if (err != B::ok) return err;
        *slot = static_cast<T*>(p);
        recs_.push_back({slot, kind, [](void* s) -> void* { T** t = static_cast<T**>(s); void* q = *t; *t = nullptr; return q; }});
        return B::ok;
    }

    // device memory, zeroed on the stream
    template <class T>
    error_t alloc_zero(T** slot, size_t count, typename B::stream_t stream) {
        error_t err = alloc(slot, count, MEM_DEVICE);
        if (err != B::ok || count == 0) return err;
        err = B::memset_async(*slot, 0, count * sizeof(T), stream);
        if (err != B::ok) release(slot);
        return err;
    }

    // a buffer that only grows: nothing when count <= cap; on failure the slot is null and cap is 0
    template <class T>
    error_t grow(T** slot, size_t& cap, size_t count, MemKind kind) {
        if (count <= cap) return B::ok;
        cap = 0;
        const error_t err = alloc(slot, count, kind);
        if (err == B::ok) cap = count;
        return err;
    }

    template <class T>
    void release(T** slot) {
        for (size_t i = recs_.size(); i-- > 0;)
            if (recs_[i].slot == slot) {
                free_slot(recs_[i]);
                recs_.erase(recs_.begin() + (std::ptrdiff_t)i);
                return;
            }
        assert(*slot == nullptr && "the slot holds a block that this owner did not allocate");
    }

    // the newest blocks down to the first `mark` (a live() taken earlier: what a routine that failed half-way has allocated since)
    void release_to(size_t mark) {
        while (recs_.size() > mark) {
            free_slot(recs_.back());
            recs_.pop_back();
        }
    }
    void release_all() { release_to(0); }       // every live block once, newest first; every slot null afterwards

    size_t live() const { return recs_.size(); }

private:
    struct Rec {
        void* slot;                 // address of the T* member
        MemKind kind;
        void* (*take)(void*);       // the slot's block, leaving the slot null (typed: no T** is ever read as a void**)
    };
    static void free_slot(const Rec& r) {
        void* p = r.take(r.slot);
        if (!p) return;
        if (r.kind == MEM_DEVICE) B::device_free(p); else B::pinned_free(p);
    }
    std::vector<Rec> recs_;
};

}  // namespace frl
