// block_layout.h — the layout of one call's device block: typed pieces, 8-byte aligned, in declaration order.
// Host-only arithmetic, no HIP: capi_ctx.h adds the device side (Block), tests/cpp/block_layout.cpp checks the offsets.
#pragma once
#include <cstddef>
#include <type_traits>

namespace svo {

template <class T>
struct Slot { size_t off, count; };  // `count` elements of T at byte `off` of the block

// A piece is declared once: the pointer that receives its device address (of the element's type), host array, count
struct BlockLayout {
    template <class P>
    using Elem = std::remove_cv_t<std::remove_pointer_t<P>>;
    // a non-empty piece with a host side: uploaded from src, downloaded to dst (either may be null)
    struct Copy { size_t off, bytes; const void* src; void* dst; };
    struct Bind { void* field; size_t off; };  // *field = block + off, once the block has an address
    static constexpr int kMaxPieces = 32;
    Copy copies[kMaxPieces];
    Bind binds[kMaxPieces];
    int n_copies = 0, n_binds = 0;
    bool overflow = false;  // a piece past kMaxPieces was dropped: Block::alloc fails
    // A staged call declares its inputs, then its outputs, then its device-only pieces, and moves [0, in_end) up and
    // [out_begin, out_end) down in one copy each (an in-out piece is the last input and the first output).
    size_t total = 0, in_end = 0, out_begin = 0, out_end = 0;

    template <class P>
    Slot<Elem<P>> in(P* field, const Elem<P>* src, size_t count) { return add(field, count, count, src, nullptr, 1); }
    // room > count: the piece takes the space of `room` elements (the copy stays `count`); a null dst is not copied
    template <class P>
    Slot<Elem<P>> out(P* field, Elem<P>* dst, size_t count, size_t room = 0) {
        return add(field, count, room > count ? room : count, nullptr, dst, 2);
    }
    template <class P>
    Slot<Elem<P>> inout(P* field, Elem<P>* io, size_t count) { return add(field, count, count, io, io, 3); }
    template <class P>
    Slot<Elem<P>> dev(P* field, size_t count) { return add(field, count, count, nullptr, nullptr, 0); }

  private:
    bool any_out_ = false;
    template <class P>
    Slot<Elem<P>> add(P* field, size_t count, size_t room, const void* src, void* dst, int dir) {
        static_assert(std::is_pointer<P>::value, "field is the pointer that receives the piece's address");
        const size_t off = total, bytes = count * sizeof(Elem<P>);
        total += (room * sizeof(Elem<P>) + 7) / 8 * 8;
        if (dir & 1) in_end = total;
        if ((dir & 2) && !any_out_) out_begin = off;
        if (dir & 2) out_end = total, any_out_ = true;
        if (n_binds == kMaxPieces) return overflow = true, Slot<Elem<P>>{off, 0};
        binds[n_binds++] = Bind{field, off};
        if (bytes && (src || dst)) copies[n_copies++] = Copy{off, bytes, src, dst};
        return Slot<Elem<P>>{off, count};
    }
};

}  // namespace svo
