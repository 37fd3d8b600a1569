// car_workspace.h — the one rule by which a caller's buffer is cut into pieces.  Host-only, plain C++ (no HIP types).
//
// A layout is ONE function that walks a Carver: run over no base it yields the total a size entry returns, run over the caller's buffer
// it yields the pointers the launcher uses, so the two cannot drift.  Pieces follow each other in the order taken; a piece's element
// count is rounded up to the layout's granule (or the take's own), which is how today's layouts differ: 64 elements in most units, 16
// bytes in car_pose.hip, none where a piece is the last one.  Offsets are computed as integers, never as arithmetic on a null pointer.
#pragma once
#include <stddef.h>
#include <stdint.h>

class Carver {
public:
    // round: the granule, in elements of the piece taken; capacity: the bytes the range holds (a sub-range's is checked, see ok())
    explicit Carver(const void* base = nullptr, size_t round = 1, size_t capacity = SIZE_MAX)
        : base_((uintptr_t)base), round_(round), cap_(capacity) {}
    // the next piece, count elements of T: its address (over no base: its byte offset as a pointer value); null when it does not fit
    template <class T>
    T* take(size_t count, size_t round = 0) {
        size_t off;
        return put(count, sizeof(T), round, &off) ? reinterpret_cast<T*>(base_ + off) : nullptr;
    }
    // the same piece as an index in elements of T from the base (for layouts that are handed out as offsets)
    template <class T>
    size_t at(size_t count, size_t round = 0) {
        size_t off = 0;
        put(count, sizeof(T), round, &off);
        return off / sizeof(T);
    }
    // pads up to a multiple of `bytes` from the base: for a piece whose start, not the size of the one before it, is what is rounded
    void align(size_t bytes) { used_ = (used_ + bytes - 1) / bytes * bytes; }
    // a piece of exactly `bytes` as a range of its own, for a nested layout: what is taken from it lies inside the piece or fails
    Carver sub(size_t bytes, size_t round = 1) {
        size_t off;
        const bool fits = put(bytes, 1, 1, &off);
        return Carver(reinterpret_cast<const void*>(base_ + (fits ? off : 0)), round, fits ? bytes : 0);
    }
    size_t bytes() const { return used_; }                             // the total so far, roundings included
    bool ok() const { return ok_; }                                    // false once a piece did not fit: that piece was not carved

private:
    bool put(size_t count, size_t size, size_t round, size_t* off) {
        const size_t r = round ? round : round_, n = (count + r - 1) / r * r * size;
        if (n > cap_ - used_) return ok_ = false;
        *off = used_;
        used_ += n;
        return true;
    }
    uintptr_t base_;
    size_t round_, cap_, used_ = 0;
    bool ok_ = true;
};
