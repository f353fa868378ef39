// nfp_torch.cpp — C++ autograd nodes over the C ABI of libnfp_hip.so (include/nfp.h).
//
// The reference's NFP is a chain of ATen ops whose autograd graph PyTorch builds (nfp.py:132-159); here one
// forward and one backward kernel stand for it, and these torch::autograd::Function classes are the graph
// nodes.  They do what functional.py's Python autograd.Functions do — allocate out / saved / grad_x, take torch's
// current stream, call nfp_forward / nfp_backward (nfp_pool_* / nfp_gap_* / nfp_valid_* / nfp_strided_* / nfp_valid_abs_*) — without the Python
// interpreter on the launch path: eager host cost per forward + backward drops from ~75 us to the autograd
// engine's own (scripts/host_overhead.py).  No device code in this file; plain pointers go across the ABI.
//
// Built by neighbour_feature_pooling_amd/build.py::build_torch_ext (g++ against libtorch + libnfp_hip.so);
// optional: functional.py falls back to its Python nodes when the module is absent.
#include <torch/extension.h>

#include <c10/hip/HIPStream.h>

#include "../../include/nfp.h"

namespace {

using torch::Tensor;
using torch::autograd::AutogradContext;
using torch::autograd::variable_list;

void check(int rc) {
  if (rc == NFP_OK) return;
  // the Python binding maps the prefix back onto NfpUnsupported / NfpError
  TORCH_CHECK(false, rc == NFP_E_UNSUPPORTED ? "libnfp_hip unsupported: " : "libnfp_hip error: ", nfp_last_error());
}

void* stream_of(const Tensor& x) { return (void*)c10::hip::getCurrentHIPStream(x.device().index()).stream(); }

Tensor empty_like_layout(const Tensor& x, bool nhwc) {
  return torch::empty(x.sizes(), x.options().memory_format(nhwc ? at::MemoryFormat::ChannelsLast : at::MemoryFormat::Contiguous));
}

// desc: CPU uint8 tensor holding one nfp_desc (the plan's descriptor; functional.py keeps it alive)
const nfp_desc* desc_of(const Tensor& desc) {
  TORCH_CHECK(desc.device().is_cpu() && desc.scalar_type() == torch::kUInt8 && desc.numel() == (int64_t)sizeof(nfp_desc),
              "descriptor tensor must be ", sizeof(nfp_desc), " bytes on the CPU");
  return (const nfp_desc*)desc.data_ptr();
}

// what the nodes share: float32 options like x; grad_out contiguous in the wanted type; NULL for a `saved` without an element
at::TensorOptions f32_like(const Tensor& x) {
  return x.options().dtype(torch::kFloat32).memory_format(at::MemoryFormat::Contiguous);
}

Tensor grad_as(const Tensor& g, at::ScalarType type) {
  Tensor c = g.contiguous();
  return c.scalar_type() == type ? c : c.to(type);
}

float* saved_ptr(const Tensor& saved) { return saved.defined() && saved.numel() ? saved.data_ptr<float>() : nullptr; }

// The four "x -> maps" families (functional.py: NFP, VALID, STRIDED, VALID_ABS): their entry points behind one argument list, and
// whether the backward reads the maps and `saved` at all.
struct NfpCalls {       // nfp_forward / nfp_backward: `saved` goes without its length
  static constexpr bool reads_maps = true;
  static int fwd(const nfp_desc* d, const void* x, void* out, float* saved, int64_t, void* s) {
    return nfp_forward(d, x, out, saved, s);
  }
  static int bwd(const nfp_desc* d, const void* x, const void* go, const void* out, const float* saved, int64_t, void* gx, void* s) {
    return nfp_backward(d, x, go, out, saved, gx, s);
  }
};
struct ValidCalls {     // an unpadded layer on the valid-map kernels: `saved` with its length; ns = 0: no backward will follow
  static constexpr bool reads_maps = true;
  static int fwd(const nfp_desc* d, const void* x, void* out, float* saved, int64_t ns, void* s) {
    return nfp_valid_forward(d, x, out, saved, ns, s);
  }
  static int bwd(const nfp_desc* d, const void* x, const void* go, const void* out, const float* saved, int64_t ns, void* gx, void* s) {
    return nfp_valid_backward(d, x, go, out, saved, ns, gx, s);
  }
};
struct StridedCalls {   // a stride 2-4 layer on the strided kernels: the valid-map contract
  static constexpr bool reads_maps = true;
  static int fwd(const nfp_desc* d, const void* x, void* out, float* saved, int64_t ns, void* s) {
    return nfp_strided_forward(d, x, out, saved, ns, s);
  }
  static int bwd(const nfp_desc* d, const void* x, const void* go, const void* out, const float* saved, int64_t ns, void* gx, void* s) {
    return nfp_strided_backward(d, x, go, out, saved, ns, gx, s);
  }
};
struct ValidAbsCalls {  // ... and their L1 family (Norm p = 1 on the difference weights, EMD): the backward reads x and grad_out
  static constexpr bool reads_maps = false;   // alone, so x is all the node saves and the maps may be modified in place
  static int fwd(const nfp_desc* d, const void* x, void* out, float*, int64_t, void* s) { return nfp_valid_abs_forward(d, x, out, s); }
  static int bwd(const nfp_desc* d, const void* x, const void* go, const void*, const float*, int64_t, void* gx, void* s) {
    return nfp_valid_abs_backward(d, x, go, gx, s);
  }
};

template <class F>
struct MapsNode : torch::autograd::Function<MapsNode<F>> {
  static Tensor forward(AutogradContext* ctx, Tensor x, Tensor desc, std::vector<int64_t> oshape, int64_t ns, bool nhwc,
                        bool need_grad) {
    c10::DeviceGuard guard(x.device());
    const nfp_desc* d = desc_of(desc);
    // (d->map_f32: bf16 x with float32 maps — the torch.autocast call, include/nfp.h)
    Tensor out = torch::empty(oshape, d->map_f32 ? f32_like(x) : x.options().memory_format(at::MemoryFormat::Contiguous));
    Tensor saved = F::reads_maps ? torch::empty({ns}, f32_like(x)) : Tensor();
    check(F::fwd(d, x.data_ptr(), out.data_ptr(), saved_ptr(saved), ns, stream_of(x)));
    if (need_grad) ctx->save_for_backward(F::reads_maps ? variable_list{x, desc, out, saved} : variable_list{x, desc});
    ctx->saved_data["nhwc"] = nhwc;
    return out;
  }
  static variable_list backward(AutogradContext* ctx, variable_list grads) {
    const auto sv = ctx->get_saved_variables();
    const Tensor &x = sv[0], &desc = sv[1];
    const Tensor out = F::reads_maps ? sv[2] : Tensor(), saved = F::reads_maps ? sv[3] : Tensor();
    c10::DeviceGuard guard(x.device());
    Tensor go = grad_as(grads[0], F::reads_maps ? out.scalar_type() : x.scalar_type());   // (the maps' type: x's, or float32)
    Tensor gx = empty_like_layout(x, ctx->saved_data["nhwc"].toBool());
    check(F::bwd(desc_of(desc), x.data_ptr(), go.data_ptr(), F::reads_maps ? out.data_ptr() : nullptr, saved_ptr(saved),
                 saved.defined() ? saved.numel() : 0, gx.data_ptr(), stream_of(x)));
    return {gx, Tensor(), Tensor(), Tensor(), Tensor(), Tensor()};
  }
};

// want_gap: GAP(x) is part of the result (NFP_Pooling.py:27); false: the pooled NFP maps alone (texture_pooling.py:251-252)
// — an empty tensor stands in for it.  need_grad: a backward will follow — only then are the maps themselves stored.
struct NfpPoolNode : torch::autograd::Function<NfpPoolNode> {
  static variable_list forward(AutogradContext* ctx, Tensor x, Tensor desc, std::vector<int64_t> oshape, int64_t ns,
                               bool nhwc, bool want_gap, bool need_grad) {
    c10::DeviceGuard guard(x.device());
    const auto f32 = f32_like(x);
    Tensor gap = torch::empty({want_gap ? oshape[0] : 0, x.size(1)}, f32), nfpm = torch::empty({oshape[0], oshape[1]}, f32);
    Tensor omap = need_grad ? torch::empty(oshape, x.options().memory_format(at::MemoryFormat::Contiguous))
                            : torch::empty({0}, x.options());
    Tensor saved = torch::empty({ns}, f32);
    check(nfp_pool_forward(desc_of(desc), x.data_ptr(), want_gap ? gap.data_ptr<float>() : nullptr, nfpm.data_ptr<float>(),
                           need_grad ? omap.data_ptr() : nullptr, saved_ptr(saved), stream_of(x)));
    ctx->save_for_backward({x, omap, saved, desc});
    ctx->saved_data["nhwc"] = nhwc;
    ctx->saved_data["want_gap"] = want_gap;
    return {gap, nfpm};
  }
  static variable_list backward(AutogradContext* ctx, variable_list grads) {
    const auto sv = ctx->get_saved_variables();
    const Tensor &x = sv[0], &omap = sv[1], &saved = sv[2], &desc = sv[3];
    c10::DeviceGuard guard(x.device());
    // a pooled output that took no part in the loss arrives undefined: its gradient is zero
    // (grad_gap = NULL: GAP(x) was not produced, or took no part in the loss — no adjoint of the mean, include/nfp.h)
    const bool has_gap = ctx->saved_data["want_gap"].toBool() && grads[0].defined();
    Tensor ggap = has_gap ? grad_as(grads[0], torch::kFloat32) : Tensor();
    Tensor gnfp = grads[1].defined() ? grad_as(grads[1], torch::kFloat32) : torch::zeros({omap.size(0), omap.size(1)}, f32_like(x));
    Tensor gx = empty_like_layout(x, ctx->saved_data["nhwc"].toBool());
    check(nfp_pool_backward(desc_of(desc), x.data_ptr(), has_gap ? ggap.data_ptr<float>() : nullptr, gnfp.data_ptr<float>(),
                            omap.data_ptr(), saved_ptr(saved), gx.data_ptr(), stream_of(x)));
    return {gx, Tensor(), Tensor(), Tensor(), Tensor(), Tensor(), Tensor()};
  }
};

// GAP(x) beside the full maps (nfp_gap_forward / nfp_gap_backward): one radius, or radii (1, 2) together (desc.inner_R).
// An output that took no part in the loss arrives undefined (set_materialize_grads(false)): gap undefined -> grad_gap =
// NULL, maps undefined -> a zero map, both undefined -> no launch.
struct NfpGapNode : torch::autograd::Function<NfpGapNode> {
  static variable_list forward(AutogradContext* ctx, Tensor x, Tensor desc, std::vector<int64_t> oshape, int64_t ns, bool nhwc) {
    c10::DeviceGuard guard(x.device());
    Tensor gap = torch::empty({x.size(0), x.size(1)}, f32_like(x));
    Tensor maps = torch::empty(oshape, x.options().memory_format(at::MemoryFormat::Contiguous));
    Tensor saved = torch::empty({ns > 0 ? ns : 1}, f32_like(x));
    check(nfp_gap_forward(desc_of(desc), x.data_ptr(), gap.data_ptr<float>(), maps.data_ptr(), saved.data_ptr<float>(),
                          saved.numel(), stream_of(x)));
    ctx->set_materialize_grads(false);
    ctx->save_for_backward({x, maps, saved, desc});
    ctx->saved_data["nhwc"] = nhwc;
    return {gap, maps};
  }
  static variable_list backward(AutogradContext* ctx, variable_list grads) {
    if (!grads[0].defined() && !grads[1].defined()) return {Tensor(), Tensor(), Tensor(), Tensor(), Tensor()};
    const auto sv = ctx->get_saved_variables();
    const Tensor &x = sv[0], &maps = sv[1], &saved = sv[2], &desc = sv[3];
    c10::DeviceGuard guard(x.device());
    const bool has_gap = grads[0].defined();
    Tensor ggap = has_gap ? grad_as(grads[0], torch::kFloat32) : Tensor();
    Tensor go = grads[1].defined() ? grad_as(grads[1], x.scalar_type()) : torch::zeros_like(maps);
    Tensor gx = empty_like_layout(x, ctx->saved_data["nhwc"].toBool());
    check(nfp_gap_backward(desc_of(desc), x.data_ptr(), has_gap ? ggap.data_ptr<float>() : nullptr, go.data_ptr(),
                           maps.data_ptr(), saved.data_ptr<float>(), saved.numel(), gx.data_ptr(), stream_of(x)));
    return {gx, Tensor(), Tensor(), Tensor(), Tensor()};
  }
};

Tensor nfp_apply(Tensor x, Tensor desc, std::vector<int64_t> oshape, int64_t ns, bool nhwc) {
  return MapsNode<NfpCalls>::apply(x, desc, oshape, ns, nhwc, true);
}
Tensor nfp_valid_apply(Tensor x, Tensor desc, std::vector<int64_t> oshape, int64_t ns, bool nhwc) {
  return MapsNode<ValidCalls>::apply(x, desc, oshape, ns, nhwc, true);
}
Tensor nfp_strided_apply(Tensor x, Tensor desc, std::vector<int64_t> oshape, int64_t ns, bool nhwc) {
  return MapsNode<StridedCalls>::apply(x, desc, oshape, ns, nhwc, true);
}
Tensor nfp_valid_abs_apply(Tensor x, Tensor desc, std::vector<int64_t> oshape, bool nhwc, bool need_grad) {
  return MapsNode<ValidAbsCalls>::apply(x, desc, oshape, (int64_t)0, nhwc, need_grad);
}
std::vector<Tensor> nfp_pool_apply(Tensor x, Tensor desc, std::vector<int64_t> oshape, int64_t ns, bool nhwc, bool want_gap,
                                   bool need_grad) {
  return NfpPoolNode::apply(x, desc, oshape, ns, nhwc, want_gap, need_grad);
}
std::vector<Tensor> nfp_gap_apply(Tensor x, Tensor desc, std::vector<int64_t> oshape, int64_t ns, bool nhwc) {
  return NfpGapNode::apply(x, desc, oshape, ns, nhwc);
}

}  // namespace

PYBIND11_MODULE(TORCH_EXTENSION_NAME, m) {
  m.def("nfp_apply", &nfp_apply, "NFPPooling.forward as one autograd node (nfp_forward / nfp_backward)");
  m.def("nfp_pool_apply", &nfp_pool_apply, "the fused nfp_pooling tail as one autograd node (nfp_pool_forward / _backward)");
  m.def("nfp_gap_apply", &nfp_gap_apply, "GAP(x) beside the full maps as one autograd node (nfp_gap_forward / _backward)");
  m.def("nfp_valid_apply", &nfp_valid_apply, "an unpadded layer's maps as one autograd node (nfp_valid_forward / _backward)");
  m.def("nfp_strided_apply", &nfp_strided_apply, "a stride 2-4 layer's maps as one autograd node (nfp_strided_forward / _backward)");
  m.def("nfp_valid_abs_apply", &nfp_valid_abs_apply,
        "an unpadded L1 layer's maps as one autograd node that saves x alone (nfp_valid_abs_forward / _backward)");
  m.attr("desc_bytes") = (int64_t)sizeof(nfp_desc);
}
