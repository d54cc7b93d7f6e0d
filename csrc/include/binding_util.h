// Helpers shared by the dispatcher bindings (csrc/bindings/*.cpp).
//
// A binding unit is host-only: it validates shapes / dtypes, allocates outputs with the caching
// allocator, picks the current HIP stream and calls the launchers declared in rn_api.h.  Each unit
// registers its own ops under torch.ops.replicann.* (TORCH_LIBRARY_FRAGMENT + TORCH_LIBRARY_IMPL in
// the same file) for the CUDA (= HIP on ROCm) dispatch key only: there is no CPU kernel — CPU tensors
// never reach these ops (ATen path in Python).
#pragma once
#include <ATen/ATen.h>
#include <ATen/hip/impl/HIPGuardImplMasqueradingAsCUDA.h>
#include <ATen/hip/impl/HIPStreamMasqueradingAsCUDA.h>
#include <hip/hip_runtime.h>
#include <torch/library.h>

#include <cstdint>
#include <optional>
#include <tuple>
#include <vector>

using at::Tensor;
using c10::optional;

inline hipStream_t cur_stream() { return c10::hip::getCurrentHIPStreamMasqueradingAsCUDA().stream(); }

#define CHECK_BF16(t) TORCH_CHECK((t).scalar_type() == at::kBFloat16, #t " must be bfloat16, got ", (t).scalar_type())
#define CHECK_CUDA(t) TORCH_CHECK((t).is_cuda(), #t " must be a GPU tensor")
#define CHECK_CONTIG(t) TORCH_CHECK((t).is_contiguous(), #t " must be contiguous")
#define GUARD(t) c10::hip::HIPGuardMasqueradingAsCUDA _guard((t).device())

// an optional tensor argument that was given
inline bool has(const optional<Tensor>& t) { return t && t->defined(); }

inline const void* optr(const optional<Tensor>& t) { return has(t) ? t->data_ptr() : nullptr; }

// seed_buf: optional 1-element int64 DEVICE tensor (from rng_next) — the kernel reads its seed there,
// so a captured hipGraph replays with a fresh draw each step
inline const uint64_t* seed_ptr(const optional<Tensor>& sb) {
    if (!has(sb)) return nullptr;
    TORCH_CHECK(sb->scalar_type() == at::kLong && sb->numel() >= 1 && sb->is_cuda(), "seed_buf: 1-element int64 GPU tensor");
    return (const uint64_t*)sb->data_ptr();
}

// a 5-D bf16 tensor whose head rows the kernels move as 16-byte vectors: an aligned base, a unit last stride and
// every other stride a non-negative multiple of 8 elements; returns the first four strides
inline std::vector<long> strides_rows16(const char* op, const char* what, const Tensor& t) {
    TORCH_CHECK(t.dim() == 5, op, ": ", what, " must have 5 dimensions, got ", t.sizes());
    TORCH_CHECK(reinterpret_cast<uintptr_t>(t.data_ptr()) % 16 == 0 && t.stride(4) == 1, op, ": ", what,
                " needs a 16-byte aligned base and a contiguous head dimension");
    std::vector<long> s;
    for (int d = 0; d < 4; ++d) {
        TORCH_CHECK(t.stride(d) % 8 == 0 && t.stride(d) >= 0, op, ": ", what, " strides must be multiples of 8 elements, got ",
                    t.strides());
        s.push_back(t.stride(d));
    }
    return s;
}

// n contiguous int32 / int64 values on `dev` (lengths, positions: the kernels clamp them)
inline void check_index(const char* op, const char* what, const Tensor& t, int64_t n, const c10::Device& dev) {
    TORCH_CHECK(t.dim() == 1 && t.size(0) == n && t.is_contiguous(), op, ": ", what, " must be a contiguous (", n,
                ",) tensor, got ", t.sizes());
    TORCH_CHECK(t.scalar_type() == at::kInt || t.scalar_type() == at::kLong, op, ": ", what,
                " must be int32 or int64, got ", t.scalar_type());
    TORCH_CHECK(t.device() == dev, op, ": ", what, " must be on ", dev);
}

inline void strides_bth(const Tensor& t, std::vector<long>& s) {
    TORCH_CHECK(t.dim() == 4 && t.stride(3) == 1, "attention tensors must be (B, T, H, D) with unit D stride");
    s.push_back(t.stride(0)); s.push_back(t.stride(1)); s.push_back(t.stride(2));
}
