// Attention and decoding bindings: attn_fwd and the backward forms, attn_decode, attn_window, linear_kv,
// sample_logits, replicann_spec::verify, replicann_kv8::attn_decode / append, replicann_prefix::attn_decode (kernels:
// attention*.hip, attention_decode.hip, attention_decode_kv8.hip, attention_decode_prefix.hip, attention_window.hip,
// gemm_skinny.hip, sampling.hip, spec_verify.hip).  Not named attention.cpp:
// the build keys its per-unit compiler flags by file stem, and those of attention.hip are for device code.
#include "binding_util.h"
#include "rn_api.h"

namespace {

// decode-step QKV projection with the K|V cache append fused into the epilogue (gemm_skinny.hip):
// x (M, K), w (N, K), kv (M, L, 2, H, D) contiguous cache, pos: int64 device row index, 1 element
// (shared by the batch) or M (one per batch row); a position outside [0, L) appends nothing
Tensor linear_kv(const Tensor& x, const Tensor& w, const optional<Tensor>& bias, const Tensor& kv, const Tensor& pos) {
    CHECK_CUDA(x); CHECK_BF16(x); CHECK_BF16(w); CHECK_BF16(kv); GUARD(x);
    TORCH_CHECK(x.dim() == 2 && x.stride(1) == 1 && w.dim() == 2 && w.stride(1) == 1, "linear_kv: 2-D row-major operands");
    const int64_t M = x.size(0), K = x.size(1), N = w.size(0);
    TORCH_CHECK(w.size(1) == K, "linear_kv: inner dims differ");
    TORCH_CHECK(kv.dim() == 5 && kv.is_contiguous() && kv.size(0) == M && kv.size(2) == 2, "linear_kv: kv must be (M, L, 2, H, D)");
    const int64_t kvw = kv.size(2) * kv.size(3) * kv.size(4);
    TORCH_CHECK(kvw <= N, "linear_kv: cache row wider than the projection");
    TORCH_CHECK(pos.scalar_type() == at::kLong && (pos.numel() == 1 || pos.numel() == M) && pos.is_contiguous() &&
                    pos.is_cuda(),
                "linear_kv: pos must be 1 or M contiguous int64 values on the device");
    TORCH_CHECK(kv.size(1) >= 1 && kv.size(1) <= (int64_t)1 << 30,"linear_kv: cache length out of range");
    TORCH_CHECK(w.device() == x.device() && kv.device() == x.device() && pos.device() == x.device() &&
                    (!has(bias) || bias->device() == x.device()),
                "linear_kv: x, w, bias, kv and pos must be on one device");
    if (has(bias)) { CHECK_BF16(*bias); TORCH_CHECK(bias->numel() == N && bias->is_contiguous()); }
    Tensor c = at::empty({M, N}, x.options());
    const int rc = rn_gemm_skinny_kv(x.data_ptr(), w.data_ptr(), optr(bias), c.data_ptr(), (int)M, (int)N, (int)K,
                                     x.stride(0), w.stride(0), c.stride(0), kv.data_ptr(), pos.data_ptr<int64_t>(),
                                     pos.numel() == 1 ? 0 : 1, (int)kv.size(1), kv.stride(0), kv.stride(1),
                                     (int)(N - kvw), cur_stream());
    TORCH_CHECK(rc == 0, "linear_kv: unsupported shape M=", M, " K=", K, " (M <= 64, K % 8 == 0)");
    return c;
}

// one-query attention over a KV cache (decode step, attention_decode.hip): q (B, 1, H, 64), k / v
// (B, Tk, H, 64) strided views, mask: Tk fp32 additive shared by the batch (or none); lens (instead
// of a mask): (B,) int32 / int64 key counts, batch row b attends to keys 0 .. lens[b]-1 only
Tensor attn_decode(const Tensor& q, const Tensor& k, const Tensor& v, const optional<Tensor>& mask, double scale,
                   const optional<Tensor>& lens) {
    CHECK_BF16(q); CHECK_BF16(k); CHECK_BF16(v); GUARD(q);
    TORCH_CHECK(q.dim() == 4 && q.size(1) == 1, "attn_decode: one query per (batch, head)");
    const int B = q.size(0), H = q.size(2), D = q.size(3), Tk = k.size(1);
    TORCH_CHECK(k.dim() == 4 && v.dim() == 4, "attn_decode: k / v must be (B, Tk, H, D)");
    TORCH_CHECK(k.size(0) == B && v.size(0) == B && k.size(2) == H && v.size(2) == H && v.size(1) == Tk &&
                    k.size(3) == D && v.size(3) == D,
                "attn_decode: shape mismatch (q ", q.sizes(), ", k ", k.sizes(), ", v ", v.sizes(), ")");
    TORCH_CHECK(k.device() == q.device() && v.device() == q.device(), "attn_decode: q, k, v on different devices");
    // the kernel reads 16-B vectors: base pointers and every non-unit stride 16-B aligned
    for (const Tensor* t : {&q, &k, &v})
        TORCH_CHECK(reinterpret_cast<uintptr_t>(t->data_ptr()) % 16 == 0 && t->stride(3) == 1,
                    "attn_decode: q / k / v need a 16-byte aligned base and a contiguous head dimension");
    if (has(mask))
        TORCH_CHECK(mask->scalar_type() == at::kFloat && mask->is_contiguous() && mask->numel() == Tk &&
                        mask->device() == q.device(),
                    "attn_decode: mask must be Tk contiguous fp32 values on q's device");
    const bool has_lens = has(lens);
    if (has_lens) {
        TORCH_CHECK(!has(mask), "attn_decode: lens cannot be combined with a mask");
        TORCH_CHECK(lens->dim() == 1 && lens->size(0) == B && lens->is_contiguous(),
                    "attn_decode: lens must be a contiguous (B,) tensor, got ", lens->sizes());
        TORCH_CHECK(lens->scalar_type() == at::kInt || lens->scalar_type() == at::kLong,
                    "attn_decode: lens must be int32 or int64, got ", lens->scalar_type());
        TORCH_CHECK(lens->device() == q.device(), "attn_decode: lens must be on q's device");
    }
    Tensor o = at::empty({B, 1, H, D}, q.options());
    std::vector<long> s;
    std::vector<long> t;
    strides_bth(q, t); s.push_back(t[0]); s.push_back(t[2]); t.clear();
    strides_bth(k, t); s.insert(s.end(), t.begin(), t.end()); t.clear();
    strides_bth(v, t); s.insert(s.end(), t.begin(), t.end()); t.clear();
    strides_bth(o, t); s.push_back(t[0]); s.push_back(t[2]);
    const int rc = rn_attn_decode(q.data_ptr(), k.data_ptr(), v.data_ptr(),
                                  has(mask) ? mask->data_ptr<float>() : nullptr,
                                  has_lens ? lens->data_ptr() : nullptr,
                                  has_lens && lens->scalar_type() == at::kLong ? 1 : 0, o.data_ptr(), B, H, Tk, D,
                                  s.data(), (float)scale, cur_stream());
    TORCH_CHECK(rc == 0, "attn_decode: unsupported shape D=", D, " Tk=", Tk, " (D == 64, Tk <= 1024)");
    return o;
}

// window attention with the cache append folded in (attention_window.hip): qkv (B, T, 3, H, 64), possibly a
// strided view of the projection output; kv (B, L, 2, H, 64) the layer's cache buffer; pos (B,) int32 / int64
// first write rows (clamped to [0, L] on the device) -> o (B, T, H, 64).  Query i of row b attends cache
// rows < pos[b] and window rows <= i; window rows that fit are written to kv[b, pos[b] + i].
Tensor attn_window(const Tensor& qkv, Tensor& kv, const Tensor& pos, double scale) {
    CHECK_CUDA(qkv); CHECK_BF16(qkv); CHECK_BF16(kv); GUARD(qkv);
    TORCH_CHECK(qkv.dim() == 5 && qkv.size(2) == 3, "attn_window: qkv must be (B, T, 3, H, D), got ", qkv.sizes());
    const int64_t B = qkv.size(0), T = qkv.size(1), H = qkv.size(3), D = qkv.size(4);
    TORCH_CHECK(kv.dim() == 5 && kv.size(0) == B && kv.size(2) == 2 && kv.size(3) == H && kv.size(4) == D,
                "attn_window: kv must be (B, L, 2, H, D) for qkv ", qkv.sizes(), ", got ", kv.sizes());
    const int64_t L = kv.size(1);
    TORCH_CHECK(T >= 1 && T <= 16, "attn_window: T = ", T, " outside 1..16");
    TORCH_CHECK(D == 64, "attn_window: head size ", D, " (64 only)");
    TORCH_CHECK(L >= 1 && L <= 1024, "attn_window: cache length ", L, " outside 1..1024");
    TORCH_CHECK(H >= 1 && B * H <= (int64_t)1 << 30, "attn_window: B * H out of range");
    TORCH_CHECK(pos.dim() == 1 && pos.size(0) == B && pos.is_contiguous(),
                "attn_window: pos must be a contiguous (B,) tensor, got ", pos.sizes());
    TORCH_CHECK(pos.scalar_type() == at::kInt || pos.scalar_type() == at::kLong,
                "attn_window: pos must be int32 or int64, got ", pos.scalar_type());
    TORCH_CHECK(kv.device() == qkv.device() && pos.device() == qkv.device(),
                "attn_window: qkv, kv and pos must be on one device");
    // the kernel moves 16-B vectors: base pointers and every non-unit stride 16-B aligned
    std::vector<long> qs, cs;
    for (int d : {0, 1, 2, 3}) { qs.push_back(qkv.stride(d)); cs.push_back(kv.stride(d)); }
    for (const Tensor* t : {&qkv, static_cast<const Tensor*>(&kv)}) {
        TORCH_CHECK(reinterpret_cast<uintptr_t>(t->data_ptr()) % 16 == 0 && t->stride(4) == 1,
                    "attn_window: qkv / kv need a 16-byte aligned base and a contiguous head dimension");
        for (int d = 0; d < 4; ++d)
            TORCH_CHECK(t->stride(d) % 8 == 0 && t->stride(d) >= 0, "attn_window: qkv / kv strides must be multiples of 8 elements");
    }
    // the append writes through kv's strides: its rows must not overlap
    TORCH_CHECK(kv.stride(3) >= D && kv.stride(2) >= H * kv.stride(3) && kv.stride(1) >= 2 * kv.stride(2) &&
                    (B == 1 || kv.stride(0) >= L * kv.stride(1)),
                "attn_window: kv must be a dense (B, L, 2, H, D) layout, got strides ", kv.strides());
    Tensor o = at::empty({B, T, H, D}, qkv.options());
    if (B == 0) return o;
    const int rc = rn_attn_window(qkv.data_ptr(), kv.data_ptr(), pos.data_ptr(), pos.scalar_type() == at::kLong ? 1 : 0,
                                  o.data_ptr(), (int)B, (int)T, (int)H, (int)L, (int)D, qs.data(), cs.data(),
                                  (float)scale, cur_stream());
    TORCH_CHECK(rc == 0, "attn_window: unsupported shape T=", T, " D=", D, " L=", L);
    return o;
}

// ---- the fp8 KV cache (attention_decode_kv8.hip): kv8 (B, L, 2, H, 64) uint8 e4m3 bytes, kv_scale (B, L, 2, H) fp32,
// pos 1 or B int32 / int64 write rows (clamped to [0, L] on the device)

// the checks the two ops share; returns kv8's byte strides (batch, row, k|v, head)
std::vector<long> kv8_check(const char* op, const Tensor& x, const Tensor& kv8, const Tensor& kv_scale, const Tensor& pos,
                            int64_t B, int64_t H, int64_t D) {
    TORCH_CHECK(kv8.scalar_type() == at::kByte && kv8.dim() == 5 && kv8.size(0) == B && kv8.size(2) == 2 &&
                    kv8.size(3) == H && kv8.size(4) == D,
                op, ": kv8 must be uint8 (B, L, 2, H, D) for ", x.sizes(), ", got ", kv8.sizes());
    const int64_t L = kv8.size(1);
    TORCH_CHECK(D == 64, op, ": head size ", D, " (64 only)");
    TORCH_CHECK(L >= 1 && H >= 1 && B * H <= (int64_t)1 << 30, op, ": cache shape out of range");
    TORCH_CHECK(kv_scale.scalar_type() == at::kFloat && kv_scale.is_contiguous() && kv_scale.dim() == 4 &&
                    kv_scale.size(0) == B && kv_scale.size(1) == L && kv_scale.size(2) == 2 && kv_scale.size(3) == H,
                op, ": kv_scale must be a contiguous float32 (B, L, 2, H) tensor, got ", kv_scale.sizes());
    TORCH_CHECK(pos.dim() == 1 && (pos.size(0) == 1 || pos.size(0) == B) && pos.is_contiguous(),
                op, ": pos must be a contiguous tensor of 1 or B values, got ", pos.sizes());
    TORCH_CHECK(pos.scalar_type() == at::kInt || pos.scalar_type() == at::kLong,
                op, ": pos must be int32 or int64, got ", pos.scalar_type());
    TORCH_CHECK(kv8.device() == x.device() && kv_scale.device() == x.device() && pos.device() == x.device(),
                op, ": every tensor must be on one device");
    // the kernels move 16-B vectors: base pointers and every non-unit stride 16-B aligned
    TORCH_CHECK(reinterpret_cast<uintptr_t>(x.data_ptr()) % 16 == 0 && x.stride(4) == 1 &&
                    reinterpret_cast<uintptr_t>(kv8.data_ptr()) % 16 == 0 && kv8.stride(4) == 1,
                op, ": the inputs need 16-byte aligned bases and a contiguous head dimension");
    std::vector<long> cs;
    for (int d = 0; d < 4; ++d) {
        TORCH_CHECK(x.stride(d) % 8 == 0 && x.stride(d) >= 0, op, ": input strides must be multiples of 8 elements");
        TORCH_CHECK(kv8.stride(d) % 16 == 0 && kv8.stride(d) >= 0, op, ": kv8 strides must be multiples of 16 bytes");
        cs.push_back(kv8.stride(d));
    }
    // the append writes through kv8's strides: its rows must not overlap
    TORCH_CHECK(kv8.stride(3) >= D && kv8.stride(2) >= H * kv8.stride(3) && kv8.stride(1) >= 2 * kv8.stride(2) &&
                    (B == 1 || kv8.stride(0) >= L * kv8.stride(1)),
                op, ": kv8 must be a dense (B, L, 2, H, D) layout, got strides ", kv8.strides());
    return cs;
}

// one-token attention over the fp8 cache with the append folded in: qkv (B, 1, 3, H, 64) bf16, possibly a strided
// view of the projection output -> o (B, 1, H, 64).  The new K / V rows are quantised and, if pos < L, written to
// row pos; the query attends rows 0 .. pos-1 and the new row.
Tensor attn_decode_kv8(const Tensor& qkv, Tensor& kv8, Tensor& kv_scale, const Tensor& pos, double scale) {
    CHECK_CUDA(qkv); CHECK_BF16(qkv); CHECK_CUDA(kv8); GUARD(qkv);
    TORCH_CHECK(qkv.dim() == 5 && qkv.size(1) == 1 && qkv.size(2) == 3,
                "attn_decode_kv8: qkv must be (B, 1, 3, H, D), got ", qkv.sizes());
    const int64_t B = qkv.size(0), H = qkv.size(3), D = qkv.size(4);
    const std::vector<long> cs = kv8_check("attn_decode_kv8", qkv, kv8, kv_scale, pos, B, H, D);
    const int64_t L = kv8.size(1);
    TORCH_CHECK(L <= 1024, "attn_decode_kv8: cache length ", L, " outside 1..1024");
    Tensor o = at::empty({B, 1, H, D}, qkv.options());
    if (B == 0) return o;
    const long qs[3] = {(long)qkv.stride(0), (long)qkv.stride(2), (long)qkv.stride(3)};
    const int rc = rn_attn_decode_kv8(qkv.data_ptr(), kv8.data_ptr(), kv_scale.data_ptr<float>(), pos.data_ptr(),
                                      pos.scalar_type() == at::kLong ? 1 : 0, (int)pos.size(0), o.data_ptr(), (int)B,
                                      (int)H, (int)L, (int)D, qs, cs.data(), (float)scale, cur_stream());
    TORCH_CHECK(rc == 0, "attn_decode_kv8: unsupported shape D=", D, " L=", L);
    return o;
}

// the prefill's append: kv_new (B, T, 2, H, 64) bf16 (a strided view is fine); rows pos[b] + i < L are quantised
// and written, the others skipped
void kv8_append(const Tensor& kv_new, Tensor& kv8, Tensor& kv_scale, const Tensor& pos) {
    CHECK_CUDA(kv_new); CHECK_BF16(kv_new); CHECK_CUDA(kv8); GUARD(kv_new);
    TORCH_CHECK(kv_new.dim() == 5 && kv_new.size(2) == 2, "kv8_append: kv_new must be (B, T, 2, H, D), got ",
                kv_new.sizes());
    const int64_t B = kv_new.size(0), T = kv_new.size(1), H = kv_new.size(3), D = kv_new.size(4);
    const std::vector<long> cs = kv8_check("kv8_append", kv_new, kv8, kv_scale, pos, B, H, D);
    if (B == 0 || T == 0) return;
    const long ns[4] = {(long)kv_new.stride(0), (long)kv_new.stride(1), (long)kv_new.stride(2), (long)kv_new.stride(3)};
    const int rc = rn_kv8_append(kv_new.data_ptr(), kv8.data_ptr(), kv_scale.data_ptr<float>(), pos.data_ptr(),
                                 pos.scalar_type() == at::kLong ? 1 : 0, (int)pos.size(0), (int)B, (int)T, (int)H,
                                 (int)kv8.size(1), (int)D, ns, cs.data(), cur_stream());
    TORCH_CHECK(rc == 0, "kv8_append: unsupported shape ", kv_new.sizes(), " into ", kv8.sizes());
}

// ---- n samples per prompt over a shared prompt cache (attention_decode_prefix.hip): qkv (B = G n, 1, 3, H, 64) bf16,
// possibly a strided view of the projection output; prefix_kv (G, P, 2, H, 64) the prompts' rows, read only;
// prefix_len (G,) and pos (B,) int32 / int64 (clamped to [0, P] / [0, L] on the device); kv (B, L, 2, H, 64) each row's
// own tail, written at pos -> o (B, 1, H, 64).  Row b of group b / n attends prefix rows < prefix_len, tail rows < pos
// and its new row.  The split partials' workspace is allocated here.
Tensor attn_decode_prefix(const Tensor& qkv, const Tensor& prefix_kv, const Tensor& prefix_len, Tensor& kv,
                          const Tensor& pos, double scale) {
    const char* op = "attn_decode_prefix";
    CHECK_CUDA(qkv); CHECK_BF16(qkv); CHECK_CUDA(prefix_kv); CHECK_BF16(prefix_kv); CHECK_CUDA(kv); CHECK_BF16(kv);
    GUARD(qkv);
    TORCH_CHECK(qkv.dim() == 5 && qkv.size(1) == 1 && qkv.size(2) == 3, op, ": qkv must be (B, 1, 3, H, D), got ",
                qkv.sizes());
    const int64_t B = qkv.size(0), H = qkv.size(3), D = qkv.size(4);
    TORCH_CHECK(prefix_kv.dim() == 5 && prefix_kv.size(2) == 2 && prefix_kv.size(3) == H && prefix_kv.size(4) == D,
                op, ": prefix_kv must be (G, P, 2, H, D) for qkv ", qkv.sizes(), ", got ", prefix_kv.sizes());
    TORCH_CHECK(kv.dim() == 5 && kv.size(0) == B && kv.size(2) == 2 && kv.size(3) == H && kv.size(4) == D,
                op, ": kv must be (B, L, 2, H, D) for qkv ", qkv.sizes(), ", got ", kv.sizes());
    const int64_t G = prefix_kv.size(0), P = prefix_kv.size(1), L = kv.size(1);
    TORCH_CHECK(G >= 1 && B >= 1 && B % G == 0, op, ": the batch ", B, " is not a multiple of the ", G, " prompts");
    const int64_t n = B / G;
    TORCH_CHECK(n <= 64, op, ": ", n, " samples per prompt (1..64)");
    TORCH_CHECK(D == 64, op, ": head size ", D, " (64 only)");
    TORCH_CHECK(P >= 1 && P <= 1024 && L >= 1 && L <= 1024, op, ": prefix length ", P, " / tail length ", L,
                " outside 1..1024");
    TORCH_CHECK(H >= 1 && B * H <= (int64_t)1 << 24, op, ": B * H out of range");
    TORCH_CHECK(prefix_kv.device() == qkv.device() && kv.device() == qkv.device(), op,
                ": qkv, prefix_kv and kv must be on one device");
    check_index(op, "prefix_len", prefix_len, G, qkv.device());
    check_index(op, "pos", pos, B, qkv.device());
    const std::vector<long> q4 = strides_rows16(op, "qkv", qkv), ps = strides_rows16(op, "prefix_kv", prefix_kv),
                            cs = strides_rows16(op, "kv", kv);
    // the append writes through kv's strides: its rows must not overlap
    TORCH_CHECK(kv.stride(3) >= D && kv.stride(2) >= H * kv.stride(3) && kv.stride(1) >= 2 * kv.stride(2) &&
                    (B == 1 || kv.stride(0) >= L * kv.stride(1)),
                op, ": kv must be a dense (B, L, 2, H, D) layout, got strides ", kv.strides());
    Tensor o = at::empty({B, 1, H, D}, qkv.options());
    Tensor ws = at::empty({rn_attn_prefix_ws_floats((int)G, (int)n, (int)H, (int)P)}, qkv.options().dtype(at::kFloat));
    const long qs[3] = {q4[0], q4[2], q4[3]};
    const int rc = rn_attn_decode_prefix(qkv.data_ptr(), prefix_kv.data_ptr(), prefix_len.data_ptr(),
                                         prefix_len.scalar_type() == at::kLong ? 1 : 0, kv.data_ptr(), pos.data_ptr(),
                                         pos.scalar_type() == at::kLong ? 1 : 0, ws.data_ptr<float>(), o.data_ptr(),
                                         (int)G, (int)n, (int)H, (int)P, (int)L, (int)D, qs, ps.data(), cs.data(),
                                         (float)scale, cur_stream());
    TORCH_CHECK(rc == 0, op, ": unsupported shape n=", n, " D=", D, " P=", P, " L=", L);
    return o;
}

// fused token sampler (sampling.hip): logits (B, V) bf16 / fp32 with a unit column stride and a row
// stride >= V (a column slice of a wider buffer is fine) -> (tokens (B, 1) int64, kept (B,) int32).
// Exactly one of u ((B,) fp32 uniforms) and seed_buf (row b draws hash_uniform(seed, b)); params: 3
// fp32 on the device (temperature, top_k, top_p) that override the host values, so that one captured
// graph serves every setting.
std::tuple<Tensor, Tensor> sample_logits(const Tensor& logits, double temperature, int64_t top_k, double top_p,
                                         const optional<Tensor>& u, const optional<Tensor>& seed_buf,
                                         const optional<Tensor>& params) {
    CHECK_CUDA(logits); GUARD(logits);
    TORCH_CHECK(logits.scalar_type() == at::kBFloat16 || logits.scalar_type() == at::kFloat,
                "sample_logits: logits must be bfloat16 or float32, got ", logits.scalar_type());
    TORCH_CHECK(logits.dim() == 2 && logits.size(1) >= 1, "sample_logits: logits must be (B, V >= 1), got ",
                logits.sizes());
    const int64_t B = logits.size(0), V = logits.size(1);
    TORCH_CHECK(V <= (1 << 30), "sample_logits: V = ", V, " exceeds 2^30");
    TORCH_CHECK(logits.stride(1) == 1 && (B == 1 || logits.stride(0) >= V),
                "sample_logits: logits need a unit column stride and a row stride >= V, got strides ",
                logits.strides());
    TORCH_CHECK(temperature >= 0.0 && temperature < INFINITY, "sample_logits: temperature must be finite and >= 0, got ",
                temperature);
    TORCH_CHECK(top_k >= 0, "sample_logits: top_k must be >= 0 (0 = off), got ", top_k);
    TORCH_CHECK(top_p > 0.0 && top_p <= 1.0, "sample_logits: top_p must be in (0, 1], got ", top_p);
    const bool has_u = has(u), has_seed = has(seed_buf);
    TORCH_CHECK(has_u != has_seed, "sample_logits: exactly one of u and seed_buf must be given");
    if (has_u)
        TORCH_CHECK(u->scalar_type() == at::kFloat && u->dim() == 1 && u->size(0) == B && u->is_contiguous() &&
                        u->device() == logits.device(),
                    "sample_logits: u must be a contiguous (B,) float32 tensor on the logits' device");
    const uint64_t* seed = seed_ptr(seed_buf);
    if (has_seed) TORCH_CHECK(seed_buf->device() == logits.device(), "sample_logits: seed_buf must be on the logits' device");
    const bool has_params = has(params);
    if (has_params)
        TORCH_CHECK(params->scalar_type() == at::kFloat && params->numel() == 3 && params->is_contiguous() &&
                        params->device() == logits.device(),
                    "sample_logits: params must be 3 contiguous float32 values (temperature, top_k, top_p) on the "
                    "logits' device");
    Tensor tokens = at::empty({B, 1}, logits.options().dtype(at::kLong));
    Tensor kept = at::empty({B}, logits.options().dtype(at::kInt));
    if (B == 0) return {tokens, kept};
    const int rc = rn_sample_logits(logits.data_ptr(), logits.scalar_type() == at::kBFloat16, B == 1 ? V : logits.stride(0),
                                    (int)B, (int)V, (float)temperature, (int)std::min<int64_t>(top_k, 1 << 30),
                                    (float)top_p, has_params ? params->data_ptr<float>() : nullptr,
                                    has_u ? u->data_ptr<float>() : nullptr, seed, tokens.data_ptr<int64_t>(),
                                    kept.data_ptr<int>(), cur_stream());
    TORCH_CHECK(rc == 0, "sample_logits: unsupported arguments (B=", B, ", V=", V, ")");
    return {tokens, kept};
}

// speculative sampling, verification (spec_verify.hip): target (B, K+1, V) and draft (B, K, V) logits of
// one dtype (bf16 / fp32) with a unit last stride and row strides >= V, drafts (B, K) int64 ->
// (tokens (B, K+1) int64, matched (B,) int64).  u: (B, K+1, 2) fp32 or seed_buf; params as for
// sample_logits.  check_drafts reads the drafts' range on the host (a sync: not inside a capture);
// without it a draft outside [0, V) is rejected on the device.
std::tuple<Tensor, Tensor> spec_verify(const Tensor& target, const Tensor& draft, const Tensor& drafts,
                                       double temperature, int64_t top_k, double top_p, const optional<Tensor>& u,
                                       const optional<Tensor>& seed_buf, const optional<Tensor>& params,
                                       bool check_drafts) {
    CHECK_CUDA(target); CHECK_CUDA(draft); CHECK_CUDA(drafts); GUARD(target);
    TORCH_CHECK(target.scalar_type() == at::kBFloat16 || target.scalar_type() == at::kFloat,
                "speculative_verify: logits must be bfloat16 or float32, got ", target.scalar_type());
    TORCH_CHECK(draft.scalar_type() == target.scalar_type(), "speculative_verify: target and draft logits differ in dtype: ",
                target.scalar_type(), " and ", draft.scalar_type());
    TORCH_CHECK(draft.device() == target.device() && drafts.device() == target.device(),
                "speculative_verify: target_logits, draft_logits and drafts must be on one device");
    TORCH_CHECK(target.dim() == 3 && draft.dim() == 3 && drafts.dim() == 2,
                "speculative_verify: need target (B, K+1, V), draft (B, K, V) and drafts (B, K), got ", target.sizes(),
                ", ", draft.sizes(), ", ", drafts.sizes());
    const int64_t B = target.size(0), K = target.size(1) - 1, V = target.size(2);
    TORCH_CHECK(K >= 1 && K <= 15, "speculative_verify: K must be in 1..15, got ", K);
    TORCH_CHECK(V >= 1 && V <= (1 << 30), "speculative_verify: V must be in 1..2^30, got ", V);
    TORCH_CHECK(B * (K + 1) <= (1 << 30), "speculative_verify: B · (K + 1) = ", B * (K + 1), " exceeds 2^30");
    TORCH_CHECK(draft.size(0) == B && draft.size(1) == K && draft.size(2) == V && drafts.size(0) == B &&
                    drafts.size(1) == K,
                "speculative_verify: need target (B, K+1, V), draft (B, K, V) and drafts (B, K), got ", target.sizes(),
                ", ", draft.sizes(), ", ", drafts.sizes());
    TORCH_CHECK(drafts.scalar_type() == at::kLong && drafts.is_contiguous(),
                "speculative_verify: drafts must be a contiguous int64 tensor");
    for (const Tensor* t : {&target, &draft})
        TORCH_CHECK(t->stride(2) == 1 && t->stride(1) >= V && (B == 1 || t->stride(0) >= t->size(1) * t->stride(1)),
                    "speculative_verify: logits need a unit last stride and non-overlapping rows of stride >= V, got strides ",
                    t->strides());
    TORCH_CHECK(temperature >= 0.0 && temperature < INFINITY,
                "speculative_verify: temperature must be finite and >= 0, got ", temperature);
    TORCH_CHECK(top_k >= 0, "speculative_verify: top_k must be >= 0 (0 = off), got ", top_k);
    TORCH_CHECK(top_p > 0.0 && top_p <= 1.0, "speculative_verify: top_p must be in (0, 1], got ", top_p);
    const bool has_u = has(u), has_seed = has(seed_buf);
    TORCH_CHECK(has_u != has_seed, "speculative_verify: exactly one of u and seed_buf must be given");
    if (has_u)
        TORCH_CHECK(u->scalar_type() == at::kFloat && u->dim() == 3 && u->size(0) == B && u->size(1) == K + 1 &&
                        u->size(2) == 2 && u->is_contiguous() && u->device() == target.device(),
                    "speculative_verify: u must be a contiguous (B, K+1, 2) float32 tensor on the logits' device");
    const uint64_t* seed = seed_ptr(seed_buf);
    if (has_seed)
        TORCH_CHECK(seed_buf->device() == target.device(), "speculative_verify: seed_buf must be on the logits' device");
    const bool has_params = has(params);
    if (has_params)
        TORCH_CHECK(params->scalar_type() == at::kFloat && params->numel() == 3 && params->is_contiguous() &&
                        params->device() == target.device(),
                    "speculative_verify: params must be 3 contiguous float32 values (temperature, top_k, top_p) on "
                    "the logits' device");
    Tensor tokens = at::empty({B, K + 1}, target.options().dtype(at::kLong));
    Tensor matched = at::empty({B}, target.options().dtype(at::kLong));
    if (B == 0) return {tokens, matched};
    if (check_drafts) {
        const auto [lo, hi] = at::aminmax(drafts);
        TORCH_CHECK(lo.item<int64_t>() >= 0 && hi.item<int64_t>() < V, "speculative_verify: drafts must lie in [0, ", V,
                    "), got ", lo.item<int64_t>(), " .. ", hi.item<int64_t>());
    }
    Tensor cand = at::empty({B, K + 1}, target.options().dtype(at::kInt));
    const long tld[2] = {(long)target.stride(0), (long)target.stride(1)};
    const long dld[2] = {(long)draft.stride(0), (long)draft.stride(1)};
    const int rc = rn_spec_verify(target.data_ptr(), tld, draft.data_ptr(), dld, drafts.data_ptr<int64_t>(),
                                  target.scalar_type() == at::kBFloat16, (int)B, (int)K, (int)V, (float)temperature,
                                  (int)std::min<int64_t>(top_k, 1 << 30), (float)top_p,
                                  has_params ? params->data_ptr<float>() : nullptr,
                                  has_u ? u->data_ptr<float>() : nullptr, seed,
                                  reinterpret_cast<uint32_t*>(cand.data_ptr<int>()), tokens.data_ptr<int64_t>(),
                                  matched.data_ptr<int64_t>(), cur_stream());
    TORCH_CHECK(rc == 0, "speculative_verify: unsupported arguments (B=", B, ", K=", K, ", V=", V, ")");
    return {tokens, matched};
}

std::tuple<Tensor, Tensor> attn_fwd(const Tensor& q, const Tensor& k, const Tensor& v, const optional<Tensor>& bias,
                                    double scale, bool causal, double p, int64_t seed,
                                    const optional<Tensor>& seed_buf) {
    CHECK_BF16(q); CHECK_BF16(k); CHECK_BF16(v); GUARD(q);
    const int B = q.size(0), Tq = q.size(1), H = q.size(2), D = q.size(3), Tk = k.size(1);
    Tensor o = at::empty({B, Tq, H, D}, q.options());
    Tensor lse = at::empty({B, H, Tq}, q.options().dtype(at::kFloat));
    std::vector<long> s;
    strides_bth(q, s); strides_bth(k, s); strides_bth(v, s); strides_bth(o, s);
    int bias_b = 1;
    if (has(bias)) {
        TORCH_CHECK(bias->scalar_type() == at::kFloat && bias->dim() == 3 && bias->is_contiguous());
        bias_b = bias->size(0);
    }
    if (B * H * Tq == 0) return {o, lse};
    int rc = rn_attn_fwd(q.data_ptr(), k.data_ptr(), v.data_ptr(), o.data_ptr(), lse.data_ptr<float>(),
                         has(bias) ? bias->data_ptr<float>() : nullptr, bias_b, s.data(), B, H, Tq, Tk, D,
                         (float)scale, causal, (float)p, (uint64_t)seed, seed_ptr(seed_buf), cur_stream());
    TORCH_CHECK(rc == 0, "attention: unsupported shape or failed launch (", rc, ") D=", D, " Tk=", Tk);
    return {o, lse};
}
// q8 / q8st / q8_only: see AttnArgs (attention_common.h); returns false (nothing launched) when the kernels
// cannot emit e5m2 for this shape
bool attn_bwd_impl(const Tensor& dout, const Tensor& q, const Tensor& k, const Tensor& v, const Tensor& o,
                   const Tensor& lse, const optional<Tensor>& bias, double scale, bool causal, double p, int64_t seed,
                   const Tensor& dq, const Tensor& dk, const Tensor& dv, const optional<Tensor>& qkv_bias_grad = {},
                   const optional<Tensor>& seed_buf = {}, void* q8 = nullptr, float* q8st = nullptr, bool q8_only = false) {
    GUARD(q);
    const int B = q.size(0), Tq = q.size(1), H = q.size(2), D = q.size(3), Tk = k.size(1);
    std::vector<long> s;
    for (const Tensor* t : {&q, &k, &v, &o, &dout, &dq, &dk, &dv}) strides_bth(*t, s);
    Tensor delta = at::empty({B, H, Tq}, q.options().dtype(at::kFloat));
    int bias_b = has(bias) ? bias->size(0) : 1;
    if (B * H * Tq == 0) return true;
    // packed-QKV bias gradient: per-64-row-block column partials from the kernels, then one reduction
    Tensor bsum;
    const bool want_bg = has(qkv_bias_grad);
    const int nblk = (Tq + 63) / 64;
    if (want_bg) {
        CHECK_BF16(*qkv_bias_grad);
        TORCH_CHECK(qkv_bias_grad->numel() == 3L * H * D && qkv_bias_grad->is_contiguous() && rn_attn_is_fast(D) &&
                    Tq == Tk, "qkv bias gradient: packed self-attention with head_dim 32, 64 or 128 only");
        bsum = at::empty({(int64_t)B * nblk, 3L * H * D}, q.options().dtype(at::kFloat));
    }
    Tensor q8part = q8 ? at::empty({rn_attn_q8_part_floats(B, H, Tq, Tk)}, q.options().dtype(at::kFloat)) : Tensor();
    int rc = rn_attn_bwd(dout.data_ptr(), q.data_ptr(), k.data_ptr(), v.data_ptr(), o.data_ptr(), lse.data_ptr<float>(),
                         has(bias) ? bias->data_ptr<float>() : nullptr, bias_b, dq.data_ptr(), dk.data_ptr(),
                         dv.data_ptr(), delta.data_ptr<float>(), s.data(), B, H, Tq, Tk, D, (float)scale, causal, (float)p,
                         (uint64_t)seed, seed_ptr(seed_buf), want_bg ? bsum.data_ptr<float>() : nullptr, q8, q8st,
                         q8_only ? 1 : 0, q8 ? q8part.data_ptr<float>() : nullptr, cur_stream());
    if (rc == -3 && q8) return false;
    TORCH_CHECK(rc == 0, "attention backward: unsupported shape or failed launch (", rc, ") D=", D);
    if (want_bg) {
        const int C = 3 * H * D;
        Tensor tmp = at::empty({rn_colsum_ws(C)}, q.options().dtype(at::kFloat));
        rn_colsum_f32(bsum.data_ptr<float>(), B * nblk, C, tmp.data_ptr<float>(), qkv_bias_grad->data_ptr(), 1,
                      cur_stream());
    }
    return true;
}
std::tuple<Tensor, Tensor, Tensor> attn_bwd(const Tensor& dout, const Tensor& q, const Tensor& k, const Tensor& v,
                                            const Tensor& o, const Tensor& lse, const optional<Tensor>& bias,
                                            double scale, bool causal, double p, int64_t seed,
                                            const optional<Tensor>& seed_buf) {
    Tensor dq = at::empty(q.sizes(), q.options());
    Tensor dk = at::empty(k.sizes(), k.options());
    Tensor dv = at::empty(v.sizes(), v.options());
    attn_bwd_impl(dout, q, k, v, o, lse, bias, scale, causal, p, seed, dq, dk, dv, {}, seed_buf);
    return {dq, dk, dv};
}
void attn_bwd_out(const Tensor& dout, const Tensor& q, const Tensor& k, const Tensor& v, const Tensor& o,
                  const Tensor& lse, const optional<Tensor>& bias, double scale, bool causal, double p, int64_t seed,
                  const Tensor& dq, const Tensor& dk, const Tensor& dv, const optional<Tensor>& qkv_bias_grad,
                  const optional<Tensor>& seed_buf) {
    attn_bwd_impl(dout, q, k, v, o, lse, bias, scale, causal, p, seed, dq, dk, dv, qkv_bias_grad, seed_buf);
}
// the same with the packed dQKV also (q8_only: only) written as e5m2 into q8 (uint8, dQKV's shape) with the
// delayed-scaling slot q8_state (rolled here); false = this shape cannot (nothing launched)
bool attn_bwd_out_q8(const Tensor& dout, const Tensor& q, const Tensor& k, const Tensor& v, const Tensor& o,
                     const Tensor& lse, const optional<Tensor>& bias, double scale, bool causal, double p, int64_t seed,
                     const Tensor& dq, const Tensor& dk, const Tensor& dv, const optional<Tensor>& qkv_bias_grad,
                     const optional<Tensor>& seed_buf, const Tensor& q8, const Tensor& q8_state, bool q8_only) {
    TORCH_CHECK(q8.scalar_type() == at::kByte && q8.is_cuda() && q8.device() == q.device(), "attn q8: uint8 on the device");
    TORCH_CHECK(q8_state.scalar_type() == at::kFloat && q8_state.numel() >= 4 && q8_state.device() == q.device());
    // the e5m2 image uses element offsets from dq: q8 is the byte twin of the packed dQKV dq / dk / dv view
    TORCH_CHECK(q8.numel() == 3 * dq.numel() && dq.data_ptr() < dk.data_ptr() && dk.data_ptr() < dv.data_ptr(),
                "attn q8: the e5m2 twin of a packed (B, T, 3, H, D) dQKV");
    return attn_bwd_impl(dout, q, k, v, o, lse, bias, scale, causal, p, seed, dq, dk, dv, qkv_bias_grad, seed_buf,
                         q8.data_ptr(), q8_state.data_ptr<float>(), q8_only);
}

}  // namespace

TORCH_LIBRARY_FRAGMENT(replicann, m) {
    m.def("attn_decode(Tensor q, Tensor k, Tensor v, Tensor? mask, float scale, Tensor? lens=None) -> Tensor");
    m.def("linear_kv(Tensor x, Tensor w, Tensor? bias, Tensor(a!) kv, Tensor pos) -> Tensor");
    m.def("sample_logits(Tensor logits, float temperature, int top_k, float top_p, Tensor? u, Tensor? seed_buf, "
          "Tensor? params) -> (Tensor, Tensor)");
    m.def("attn_fwd(Tensor q, Tensor k, Tensor v, Tensor? bias, float scale, bool causal, float p, int seed, "
          "Tensor? seed_buf=None) -> (Tensor, Tensor)");
    m.def("attn_bwd(Tensor dout, Tensor q, Tensor k, Tensor v, Tensor o, Tensor lse, Tensor? bias, float scale, "
          "bool causal, float p, int seed, Tensor? seed_buf=None) -> (Tensor, Tensor, Tensor)");
    m.def("attn_bwd_out(Tensor dout, Tensor q, Tensor k, Tensor v, Tensor o, Tensor lse, Tensor? bias, float scale, "
          "bool causal, float p, int seed, Tensor(a!) dq, Tensor(b!) dk, Tensor(c!) dv, "
          "Tensor(d!)? qkv_bias_grad=None, Tensor? seed_buf=None) -> ()");
    m.def("attn_bwd_out_q8(Tensor dout, Tensor q, Tensor k, Tensor v, Tensor o, Tensor lse, Tensor? bias, float scale, "
          "bool causal, float p, int seed, Tensor(a!) dq, Tensor(b!) dk, Tensor(c!) dv, "
          "Tensor(d!)? qkv_bias_grad, Tensor? seed_buf, Tensor(e!) q8, Tensor(f!) q8_state, bool q8_only) -> bool");
}

// decoding ops added after the replicann:: list was frozen live in a namespace of their own
TORCH_LIBRARY_FRAGMENT(replicann_decode, m) {
    m.def("attn_window(Tensor qkv, Tensor(a!) kv, Tensor pos, float scale) -> Tensor");
}

TORCH_LIBRARY_IMPL(replicann_decode, CUDA, m) {
    m.impl("attn_window", &attn_window);
}

// speculative sampling: a namespace of its own too (the replicann_decode:: list is frozen as well)
TORCH_LIBRARY_FRAGMENT(replicann_spec, m) {
    m.def("verify(Tensor target_logits, Tensor draft_logits, Tensor drafts, float temperature, int top_k, float top_p, "
          "Tensor? u, Tensor? seed_buf, Tensor? params, bool check_drafts) -> (Tensor, Tensor)");
}

TORCH_LIBRARY_IMPL(replicann_spec, CUDA, m) {
    m.impl("verify", &spec_verify);
}

// the fp8 KV cache: its own namespace as well (every list above is pinned by a test)
TORCH_LIBRARY_FRAGMENT(replicann_kv8, m) {
    m.def("attn_decode(Tensor qkv, Tensor(a!) kv8, Tensor(b!) kv_scale, Tensor pos, float scale) -> Tensor");
    m.def("append(Tensor kv_new, Tensor(a!) kv8, Tensor(b!) kv_scale, Tensor pos) -> ()");
}

TORCH_LIBRARY_IMPL(replicann_kv8, CUDA, m) {
    m.impl("attn_decode", &attn_decode_kv8);
    m.impl("append", &kv8_append);
}

// n samples per prompt over a shared prompt cache: the same again
TORCH_LIBRARY_FRAGMENT(replicann_prefix, m) {
    m.def("attn_decode(Tensor qkv, Tensor prefix_kv, Tensor prefix_len, Tensor(a!) kv, Tensor pos, float scale) -> Tensor");
}

TORCH_LIBRARY_IMPL(replicann_prefix, CUDA, m) {
    m.impl("attn_decode", &attn_decode_prefix);
}

TORCH_LIBRARY_IMPL(replicann, CUDA, m) {
    m.impl("attn_decode", &attn_decode);
    m.impl("linear_kv", &linear_kv);
    m.impl("sample_logits", &sample_logits);
    m.impl("attn_fwd", &attn_fwd);
    m.impl("attn_bwd", &attn_bwd);
    m.impl("attn_bwd_out", &attn_bwd_out);
    m.impl("attn_bwd_out_q8", &attn_bwd_out_q8);
}
