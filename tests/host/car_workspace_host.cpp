// Stand-alone check of csrc/car_workspace.h (tests/test_workspace_host.py builds and runs it; plain g++, no HIP).
// One layout function per case, run over no base and over a real buffer, as the library's units do.
#include "car_workspace.h"

#include <stdio.h>
#include <stdlib.h>
#include <vector>

static int g_failed = 0;
#define CHECK(cond)                                                      \
    do {                                                                 \
        if (!(cond)) { printf("FAILED %s:%d: %s\n", __FILE__, __LINE__, #cond); ++g_failed; } \
    } while (0)

struct Piece { uintptr_t at; size_t bytes, align; };

// a layout with every kind of piece: mixed types under one granule, a take with its own granule, a pad, a last piece as long as it is
struct Mixed { std::vector<Piece> pieces; size_t total; bool ok; };
static Mixed mixed(size_t n, void* base) {
    Mixed m;
    Carver c(base, 64);
    auto add = [&](void* p, size_t bytes, size_t align) { m.pieces.push_back(Piece{(uintptr_t)p, bytes, align}); };
    add(c.take<float>(n), n * 4, 256);
    add(c.take<double>(n + 1), (n + 1) * 8, 256);                    // 64 doubles: the granule counts elements, so 512 bytes here
    add(c.take<int>(3 * n, 4), 3 * n * 4, 16);
    add(c.take<char>(n, 1), n, 1);                                   // leaves the total odd: the pad below has work to do
    c.align(16);
    add(c.take<double>(n, 1), n * 8, 16);
    m.total = c.bytes();
    m.ok = c.ok();
    return m;
}

// a parent with a nested range, as car_vit_blocks' workspace holds car_mha's
struct Inner { float *a, *b; size_t total; };
static Inner inner(size_t n, void* base) {
    Carver c(base, 64);
    Inner i;
    i.a = c.take<float>(n);
    i.b = c.take<float>(2 * n, 1);
    i.total = c.bytes();
    return i;
}
struct Outer { float* head; Inner in; uintptr_t nested_at; size_t nested_bytes; float* tail; size_t total; bool ok; };
static Outer outer(size_t n, void* base) {
    Outer o;
    Carver c(base, 64);
    o.head = c.take<float>(n);
    o.nested_bytes = inner(n, nullptr).total;
    Carver sub = c.sub(o.nested_bytes);
    o.nested_at = (uintptr_t)sub.take<char>(0);
    o.in = inner(n, reinterpret_cast<void*>(o.nested_at));
    o.tail = c.take<float>(1);
    o.total = c.bytes();
    o.ok = c.ok() && sub.ok();
    return o;
}

int main() {
    for (size_t n : {(size_t)1, (size_t)3, (size_t)33, (size_t)64, (size_t)65, (size_t)1000}) {
        const Mixed size = mixed(n, nullptr);
        std::vector<char> raw(size.total + 256);
        char* base = reinterpret_cast<char*>(((uintptr_t)raw.data() + 255) / 256 * 256);
        const Mixed m = mixed(n, base);
        // totals with and without a base agree, and so does every offset
        CHECK(size.ok && m.ok && m.total == size.total && m.pieces.size() == size.pieces.size());
        uintptr_t end = (uintptr_t)base;
        for (size_t i = 0; i < m.pieces.size(); ++i) {
            const Piece& p = m.pieces[i];
            CHECK(p.at - (uintptr_t)base == size.pieces[i].at);
            CHECK(p.at % p.align == 0);                                                    // aligned as asked
            CHECK(p.at >= end);                                                            // overlaps no piece before it
            CHECK(p.at + p.bytes <= (uintptr_t)base + m.total);                            // inside the range
            end = p.at + p.bytes;
            for (size_t k = 0; k < p.bytes; ++k) reinterpret_cast<char*>(p.at)[k] = (char)i;   // under the sanitizer: every byte is the buffer's
        }
        // the roundings themselves: 64 floats, 64 doubles, 4 ints, n chars, the pad, then n doubles as they are
        const size_t up = (n + 63) / 64 * 64, up1 = (n + 1 + 63) / 64 * 64;
        CHECK(size.total == (up * 4 + up1 * 8 + (3 * n + 3) / 4 * 4 * 4 + n + 15) / 16 * 16 + n * 8);

        const Outer so = outer(n, nullptr);
        std::vector<char> raw2(so.total + 256);
        char* base2 = reinterpret_cast<char*>(((uintptr_t)raw2.data() + 255) / 256 * 256);
        const Outer o = outer(n, base2);
        CHECK(so.ok && o.ok && o.total == so.total && o.nested_bytes == so.in.total);
        // the nested layout's pieces lie inside their parent's piece, which lies between the parent's own pieces
        CHECK((uintptr_t)o.head + n * 4 <= o.nested_at && o.nested_at + o.nested_bytes <= (uintptr_t)o.tail);
        CHECK((uintptr_t)o.in.a == o.nested_at && (uintptr_t)(o.in.b + 2 * n) <= o.nested_at + o.nested_bytes);
        CHECK((uintptr_t)(o.tail + 1) <= (uintptr_t)base2 + o.total);
    }
    {   // an over-full sub-range is reported, not carved: the piece that does not fit comes back null and the range keeps its total
        char buf[256];
        Carver c(buf);
        Carver sub = c.sub(100);
        char* a = sub.take<char>(60);
        CHECK(a == buf && sub.ok());
        CHECK(sub.take<char>(41) == nullptr && !sub.ok() && sub.bytes() == 60);
        CHECK(sub.take<char>(40) == buf + 60 && sub.bytes() == 100 && !sub.ok());           // the report stays
        CHECK(c.ok() && c.bytes() == 100);
        Carver exact = c.sub(8, 2);
        CHECK(exact.take<float>(1) == (float*)(buf + 100) && exact.ok() && exact.bytes() == 8);   // one float on a granule of two: just fits
        Carver full(buf, 1, 16);
        CHECK(full.take<double>(2) == (double*)buf && full.ok() && full.take<char>(1) == nullptr && !full.ok());
        Carver past(buf, 1, 16);
        Carver none = past.sub(17);                                                          // the sub-range itself does not fit
        CHECK(!past.ok() && none.take<char>(1) == nullptr && !none.ok() && past.bytes() == 0);
    }
    if (g_failed) { printf("%d checks failed\n", g_failed); return 1; }
    printf("car_workspace: OK\n");
    return 0;
}
