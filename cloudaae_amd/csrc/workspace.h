// workspace.h -- the one place that lays regions out in a caller-allocated workspace ("Workspaces").  A layout is
// ONE function of the shape arguments and the base pointer that takes its regions from a Carver in order: the query calls it
// with a null base and returns bytes(), the launcher calls it with the workspace and uses the pointers, so the two cannot
// state different layouts.  Plain host C++, nothing of HIP: tests/workspace_carver_main.cpp compiles it alone.
#pragma once
#include <stddef.h>

namespace cloudaae {

// bytes rounded up to a multiple of align
inline size_t workspace_pad(size_t bytes, size_t align = 256) { return (bytes + align - 1) / align * align; }

struct Carver {
    char *base;                                    // may be null: every region is null then, bytes() the same
    size_t used = 0;
    explicit Carver(void *workspace) : base(static_cast<char *>(workspace)) {}

    // the next region: count elements of T, its END padded to align bytes (the next region starts aligned when the base is)
    template <typename T>
    T *take(size_t count, size_t align = 256)
    {
        T *p = base ? reinterpret_cast<T *>(base + used) : nullptr;
        used += workspace_pad(sizeof(T) * count, align);
        return p;
    }
    size_t bytes() const { return used; }
};

} // namespace cloudaae
