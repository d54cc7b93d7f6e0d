// Embedding, ViT token join and optimizer bindings (kernels: embedding_optim.hip).
#include <cstdlib>
#include <map>
#include <mutex>

#include "binding_util.h"
#include "rn_api.h"

namespace {

// ViT token join: x[b] = concat(cls, patch[b]) + pos — patch (B, P, E), cls (E), pos (P + 1, E), all bf16
Tensor vit_join_fwd(const Tensor& patch, const Tensor& cls, const Tensor& pos) {
    CHECK_BF16(patch); CHECK_CONTIG(patch); CHECK_BF16(cls); CHECK_CONTIG(cls); CHECK_BF16(pos); CHECK_CONTIG(pos);
    GUARD(patch);
    TORCH_CHECK(patch.dim() == 3, "vit_join_fwd: patch must be (B, P, E)");
    const int B = patch.size(0), P = patch.size(1), E = patch.size(2);
    TORCH_CHECK(E % 8 == 0 && cls.numel() == E && pos.numel() == (long)(P + 1) * E, "vit_join_fwd: shapes");
    Tensor out = at::empty({B, P + 1, E}, patch.options());
    if (B) rn_vit_join_fwd(patch.data_ptr(), cls.data_ptr(), pos.data_ptr(), out.data_ptr(), B, P, E, cur_stream());
    return out;
}
// backward: returns dpatch (B, P, E); gcls (E) and gpos (P + 1, E) are ACCUMULATED into (bf16)
Tensor vit_join_bwd(const Tensor& dx, const Tensor& gcls, const Tensor& gpos) {
    CHECK_BF16(dx); CHECK_CONTIG(dx); CHECK_BF16(gcls); CHECK_CONTIG(gcls); CHECK_BF16(gpos); CHECK_CONTIG(gpos);
    GUARD(dx);
    TORCH_CHECK(dx.dim() == 3, "vit_join_bwd: dx must be (B, P + 1, E)");
    const int B = dx.size(0), P = dx.size(1) - 1, E = dx.size(2);
    TORCH_CHECK(P >= 0 && E % 8 == 0 && gcls.numel() == E && gpos.numel() == (long)(P + 1) * E, "vit_join_bwd: shapes");
    Tensor dpatch = at::empty({B, P, E}, dx.options());
    if (B) rn_vit_join_bwd(dx.data_ptr(), dpatch.data_ptr(), gcls.data_ptr(), gpos.data_ptr(), B, P, E, cur_stream());
    return dpatch;
}

Tensor embedding_fwd(const Tensor& ids, const Tensor& wte, const optional<Tensor>& wpe) {
    CHECK_BF16(wte); CHECK_CONTIG(wte); GUARD(wte);
    TORCH_CHECK(ids.scalar_type() == at::kLong && ids.is_contiguous());
    const int E = wte.size(1);
    TORCH_CHECK(E % 8 == 0, "embedding width must be a multiple of 8");
    const int T = ids.dim() >= 2 ? ids.size(-1) : ids.numel();
    const int rows = ids.numel();
    if (has(wpe)) TORCH_CHECK(wpe->size(0) >= T, "sequence longer than the position table");
    auto shape = ids.sizes().vec();
    shape.push_back(E);
    Tensor x = at::empty(shape, wte.options());
    if (rows)
        rn_emb_fwd(ids.data_ptr<int64_t>(), wte.data_ptr(), optr(wpe), x.data_ptr(), rows, T, E, (int)wte.size(0),
                   cur_stream());
    return x;
}
std::tuple<Tensor, Tensor> embedding_bwd(const Tensor& dx, const Tensor& ids, int64_t V, int64_t Tp) {
    CHECK_BF16(dx); CHECK_CONTIG(dx); GUARD(dx);
    const int E = dx.size(-1);
    const int T = ids.dim() >= 2 ? ids.size(-1) : ids.numel();
    const int B = ids.numel() / std::max(T, 1);
    Tensor d32 = at::empty({V * E}, dx.options().dtype(at::kFloat));
    Tensor dwte = at::empty({V, E}, dx.options());
    Tensor dwpe = at::empty({Tp, E}, dx.options());
    rn_emb_bwd(ids.data_ptr<int64_t>(), dx.data_ptr(), d32.data_ptr<float>(), dwte.data_ptr(), Tp ? dwpe.data_ptr() : nullptr,
               B, T, (int)Tp, (int)V, E, cur_stream());
    return {dwte, dwpe};
}

// Direct-accumulate embedding backward: gwte/gwpe (flat gradient views) += scatter.
// The fp32 scratch and owner table are persistent per (device, V, E) and are left
// in their initial state by every call, so the op is hipGraph-capturable.
void embedding_bwd_acc(const Tensor& dx, const Tensor& ids, const Tensor& gwte, const optional<Tensor>& gwpe) {
    CHECK_BF16(dx); CHECK_CONTIG(dx); CHECK_BF16(gwte); CHECK_CONTIG(gwte); GUARD(dx);
    TORCH_CHECK(ids.scalar_type() == at::kLong && ids.is_contiguous());
    const int64_t V = gwte.size(0), E = gwte.size(1);
    TORCH_CHECK(dx.size(-1) == E && E % 4 == 0, "embedding_bwd_acc: width mismatch / E % 4");
    const int T = ids.dim() >= 2 ? ids.size(-1) : ids.numel();
    const int B = ids.numel() / std::max(T, 1);
    if (has(gwpe)) {
        CHECK_BF16(*gwpe); CHECK_CONTIG(*gwpe);
        TORCH_CHECK(gwpe->size(0) >= T && gwpe->size(1) == E);
    }
    // REPLICANN_DETERMINISTIC=1: 64-bit fixed-point scratch, order-independent integer atomics
    const char* de = std::getenv("REPLICANN_DETERMINISTIC");
    const bool det = de && de[0] == '1';
    static std::map<std::tuple<int, int64_t, int64_t, int>, std::pair<Tensor, Tensor>> scratch;
    static std::mutex mu;
    std::pair<Tensor, Tensor> buf;
    {
        std::lock_guard<std::mutex> lk(mu);
        auto key = std::make_tuple((int)dx.get_device(), V, E, (int)det);
        auto it = scratch.find(key);
        if (it == scratch.end()) {
            hipStreamCaptureStatus cs = hipStreamCaptureStatusNone;
            (void)hipStreamIsCapturing(cur_stream(), &cs);
            TORCH_CHECK(cs == hipStreamCaptureStatusNone,
                        "embedding_bwd_acc: first call must be eager (scratch allocation)");
            Tensor d32 = at::zeros({V * E * (det ? 2 : 1)}, dx.options().dtype(at::kFloat));
            Tensor own = at::full({V}, -1, dx.options().dtype(at::kInt));
            it = scratch.emplace(key, std::make_pair(d32, own)).first;
        }
        buf = it->second;
    }
    if (ids.numel() && det)
        rn_emb_bwd_acc_det(ids.data_ptr<int64_t>(), dx.data_ptr(), buf.first.data_ptr(),
                           reinterpret_cast<unsigned*>(buf.second.data_ptr<int>()), gwte.data_ptr(),
                           has(gwpe) ? gwpe->data_ptr() : nullptr, B, T, (int)E, (int)V, cur_stream());
    else if (ids.numel())
        rn_emb_bwd_acc(ids.data_ptr<int64_t>(), dx.data_ptr(), buf.first.data_ptr<float>(),
                       reinterpret_cast<unsigned*>(buf.second.data_ptr<int>()), gwte.data_ptr(),
                       has(gwpe) ? gwpe->data_ptr() : nullptr, B, T, (int)E, (int)V, cur_stream());
}

void sumsq(const Tensor& g, const Tensor& normbuf) {
    CHECK_CONTIG(g); GUARD(g);
    TORCH_CHECK(normbuf.scalar_type() == at::kFloat && normbuf.numel() >= 2);
    Tensor part = at::empty({rn_norm_ws_floats()}, g.options().dtype(at::kFloat));
    rn_sumsq(g.data_ptr(), g.numel(), g.scalar_type() == at::kBFloat16, part.data_ptr<float>(), normbuf.data_ptr<float>(),
             cur_stream());
}
void opt_prep(const Tensor& state, double base_lr, double warmup, double total, double min_ratio, bool cosine,
              double lr_override, double b1, double b2) {
    GUARD(state);
    TORCH_CHECK(state.scalar_type() == at::kFloat && state.numel() >= 8);
    rn_opt_prep(state.data_ptr<float>(), (float)base_lr, (float)warmup, (float)total, (float)min_ratio, cosine,
                (float)lr_override, (float)b1, (float)b2, cur_stream());
}
void adamw_step(const Tensor& p, const Tensor& master, const Tensor& g, const Tensor& m, const Tensor& v,
                const Tensor& wdm, const Tensor& state, double b1, double b2, double eps, double wd, double gscale,
                double clip, bool stochastic_round) {
    CHECK_BF16(p); GUARD(p);
    TORCH_CHECK(master.scalar_type() == at::kFloat && m.scalar_type() == at::kFloat && v.scalar_type() == at::kFloat);
    TORCH_CHECK(p.numel() == master.numel() && p.numel() == g.numel() && wdm.numel() * 64 >= p.numel());
    int rc = rn_adamw(p.data_ptr(), master.data_ptr<float>(), g.data_ptr(), g.scalar_type() == at::kBFloat16,
                      m.data_ptr<float>(), v.data_ptr<float>(), wdm.data_ptr<uint8_t>(), state.data_ptr<float>(),
                      p.numel(), (float)b1, (float)b2, (float)eps, (float)wd, (float)gscale, (float)clip,
                      stochastic_round ? 1 : 0, cur_stream());
    TORCH_CHECK(rc == 0, "adamw: flat buffer length must be a multiple of 8");
}
void sgd_step(const Tensor& p, const Tensor& master, const Tensor& g, const Tensor& buf, const Tensor& wdm,
              const Tensor& state, double mom, double wd, bool nesterov, double gscale, double clip) {
    CHECK_BF16(p); GUARD(p);
    rn_sgd(p.data_ptr(), master.data_ptr<float>(), g.data_ptr(), g.scalar_type() == at::kBFloat16, buf.data_ptr<float>(),
           wdm.data_ptr<uint8_t>(), state.data_ptr<float>(), p.numel(), (float)mom, (float)wd, nesterov, (float)gscale,
           (float)clip, cur_stream());
}

}  // namespace

TORCH_LIBRARY_FRAGMENT(replicann, m) {
    m.def("embedding_fwd(Tensor ids, Tensor wte, Tensor? wpe) -> Tensor");
    m.def("vit_join_fwd(Tensor patch, Tensor cls, Tensor pos) -> Tensor");
    m.def("vit_join_bwd(Tensor dx, Tensor(a!) gcls, Tensor(b!) gpos) -> Tensor");
    m.def("embedding_bwd(Tensor dx, Tensor ids, int V, int Tp) -> (Tensor, Tensor)");
    m.def("embedding_bwd_acc(Tensor dx, Tensor ids, Tensor(a!) gwte, Tensor(b!)? gwpe) -> ()");
    m.def("sumsq(Tensor g, Tensor(a!) normbuf) -> ()");
    m.def("opt_prep(Tensor(a!) state, float base_lr, float warmup, float total, float min_ratio, bool cosine, "
          "float lr_override, float b1, float b2) -> ()");
    m.def("adamw_step(Tensor(a!) p, Tensor(b!) master, Tensor g, Tensor(c!) m, Tensor(d!) v, Tensor wdm, Tensor(e!) state, "
          "float b1, float b2, float eps, float wd, float gscale, float clip, bool stochastic_round=False) -> ()");
    m.def("sgd_step(Tensor(a!) p, Tensor(b!) master, Tensor g, Tensor(c!) buf, Tensor wdm, Tensor(e!) state, "
          "float mom, float wd, bool nesterov, float gscale, float clip) -> ()");
}

TORCH_LIBRARY_IMPL(replicann, CUDA, m) {
    m.impl("embedding_fwd", &embedding_fwd);
    m.impl("vit_join_fwd", &vit_join_fwd);
    m.impl("vit_join_bwd", &vit_join_bwd);
    m.impl("embedding_bwd", &embedding_bwd);
    m.impl("embedding_bwd_acc", &embedding_bwd_acc);
    m.impl("sumsq", &sumsq);
    m.impl("opt_prep", &opt_prep);
    m.impl("adamw_step", &adamw_step);
    m.impl("sgd_step", &sgd_step);
}
