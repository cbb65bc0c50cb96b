// The carver of cloudaae_amd/csrc/workspace.h on the host alone (tests/test_workspace_sizes_host.py compiles this with
// -fsanitize=address,undefined and runs it): every region lies inside the block and starts aligned, a null base gives
// null pointers and the same total, a region of no elements takes no bytes, and totals above 2^32 do not wrap.
#include "workspace.h"

#include <initializer_list>
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

using cloudaae::Carver;

static int failures = 0;
#define EXPECT(cond)                                                       \
    do {                                                                   \
        if (!(cond)) {                                                     \
            printf("%s:%d: %s does not hold\n", __FILE__, __LINE__, #cond); \
            ++failures;                                                    \
        }                                                                  \
    } while (0)

struct Layout {
    double *a;
    unsigned char *b;
    int *none, *c;
    float *d;
    size_t bytes;
};

static Layout layout(void *base, size_t align)
{
    Carver ws(base);
    Layout L;
    L.a = ws.take<double>(3, align);               // 24 bytes
    L.b = ws.take<unsigned char>(257, align);
    L.none = ws.take<int>(0, align);
    L.c = ws.take<int>(65, align);
    L.d = ws.take<float>(1, align);
    L.bytes = ws.bytes();
    return L;
}

static size_t pad(size_t x, size_t align) { return (x + align - 1) / align * align; }

int main()
{
    for (size_t align : {(size_t)8, (size_t)16, (size_t)256}) {
        const Layout sizes = layout(nullptr, align);
        EXPECT(!sizes.a && !sizes.b && !sizes.none && !sizes.c && !sizes.d);
        EXPECT(sizes.bytes == pad(24, align) + pad(257, align) + pad(260, align) + pad(4, align));

        char *block = static_cast<char *>(aligned_alloc(256, pad(sizes.bytes, 256)));
        const Layout L = layout(block, align);
        EXPECT(L.bytes == sizes.bytes);
        EXPECT((char *)L.a == block);
        EXPECT((char *)L.b == block + pad(24, align));
        EXPECT((char *)L.none == (char *)L.b + pad(257, align));
        EXPECT((char *)L.c == (char *)L.none);      // no elements: no bytes, the next region starts where it would have
        EXPECT((char *)L.d == (char *)L.c + pad(260, align));
        for (const void *p : {(const void *)L.a, (const void *)L.b, (const void *)L.none, (const void *)L.c, (const void *)L.d})
            EXPECT((uintptr_t)p % align == 0);
        // every element of every region is the block's to write (the sanitizer objects otherwise)
        memset(L.a, 1, 3 * sizeof(double));
        memset(L.b, 2, 257);
        memset(L.c, 3, 65 * sizeof(int));
        memset(L.d, 4, sizeof(float));
        EXPECT((char *)(L.d + 1) <= block + sizes.bytes);
        free(block);
    }

    // the default pad is 256 bytes
    Carver dflt(nullptr);
    dflt.take<char>(1);
    EXPECT(dflt.bytes() == 256);

    // above 2^32: 2^29 doubles, then 2^30 + 1 ints
    Carver big(nullptr);
    EXPECT(big.take<double>((size_t)1 << 29) == nullptr);
    big.take<int>(((size_t)1 << 30) + 1);
    EXPECT(big.bytes() == ((size_t)1 << 32) + ((size_t)1 << 32) + 256);
    char *const far_base = reinterpret_cast<char *>((uintptr_t)1 << 40);      // (never dereferenced)
    Carver far(far_base);
    far.take<double>((size_t)1 << 29);
    EXPECT(reinterpret_cast<uintptr_t>(far.take<int>(1)) == ((uintptr_t)1 << 40) + ((uintptr_t)1 << 32));

    if (failures == 0)
        printf("workspace carver: ok\n");
    return failures == 0 ? 0 : 1;
}
