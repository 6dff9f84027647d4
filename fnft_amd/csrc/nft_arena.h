// nft_arena.h -- the one owner of device memory.  Every plan class and every host-pointer entry point holds a
// DevArena<BE> and asks it for its buffers; the arena hands the blocks back to the back end when it is cleared or goes
// out of scope, so no class keeps a list of its pointers and no function has to reach a block of be.free calls.
// It is a list of blocks, nothing more: no sub-allocation, no alignment logic, no size classes (the product's block
// cache is fa_pool_* in hip_backend.hip, behind BE::alloc).
#pragma once
#include <cstddef>
#include <vector>

template <class BE> class DevArena {
public:
    BE &be;
    size_t bytes = 0;   // requested bytes of the blocks held: what the *_workspace_bytes entries report

    explicit DevArena(BE &be_) : be(be_) {}
    DevArena(const DevArena &) = delete;
    DevArena &operator=(const DevArena &) = delete;
    ~DevArena() { clear(); }

    // count values of T (a block of 16 bytes if that is none); false, with p null, if the back end has no memory
    template <class T> bool get(T *&p, size_t count)
    {
        const size_t b = count * sizeof(T);
        p = (T *)be.alloc(b ? b : 16);
        if (!p) return false;
        bytes += b;
        blocks.push_back(Block{p, b});
        return true;
    }
    // one block back before the rest (a work array that is regrown); p becomes null.  A null p is ignored.
    template <class T> void give_back(T *&p)
    {
        for (size_t i = blocks.size(); i-- > 0;)
            if (blocks[i].p == (void *)p) {
                bytes -= blocks[i].bytes;
                be.free(blocks[i].p);
                blocks.erase(blocks.begin() + (std::ptrdiff_t)i);
                break;
            }
        p = nullptr;
    }
    void clear()
    {
        for (const Block &b : blocks) be.free(b.p);
        blocks.clear();
        bytes = 0;
    }

private:
    struct Block { void *p; size_t bytes; };
    std::vector<Block> blocks;
};
