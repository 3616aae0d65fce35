// Host-only check of the argument checks the C entry points share (edhip_api.hip: check_naxis, check_displacement,
// check_pairs, deformed_lengths, sample, fill_geometry, and what the strided-batch calls on the prefiltered grid share:
// check_batch_call, check_axes_1_to_3, check_prefiltered, check_batch_limit, has_shape, f32_or_f64, check_status,
// check_iteration, batch_array) on hostile descriptors -- no HIP call is made.  The helpers
// live in that file's anonymous namespace, so the file is included; link against libedhip.so for the launchers it
// names.  Every array is a heap block of exactly the size the ABI promises, so that a build with
// -Xarch_host -fsanitize=address,undefined reports any read beyond it.  Built and run by
// tests/test_api_checks_host.py.
#include <cmath>
#include <cstdio>
#include <cstring>
#include <memory>
#include <vector>

#include "edhip_api.hip"

#define CHECK(c)                                                          \
    do {                                                                  \
        if (!(c)) {                                                       \
            std::printf("FAILED line %d: %s\n", __LINE__, #c);            \
            return 1;                                                     \
        }                                                                 \
    } while (0)

namespace {

// a descriptor on the heap: rank, dtype code and extents as given (dense float64 strides)
std::unique_ptr<edhip_array> desc(int ndim, std::vector<int64_t> shape, int dtype = EDHIP_F32)
{
    std::unique_ptr<edhip_array> a(new edhip_array);
    memset(a.get(), 0, sizeof(edhip_array));
    a->data = (void*)0x1000;
    a->dtype = dtype;
    a->ndim = ndim;
    int64_t stride = 8;
    for (int d = (int)shape.size() - 1; d >= 0; --d) {
        a->shape[d] = shape[d];
        a->stride_bytes[d] = stride;
        stride *= shape[d] > 0 ? shape[d] : 1;
    }
    return a;
}

char msg[256];
bool said(const char* want) { return strcmp(msg, want) == 0; }

}  // namespace

int main()
{
    using namespace ed;
    const size_t n = sizeof(msg);
    // ---- check_naxis -------------------------------------------------------------------------------------------
    CHECK(check_naxis(0, msg, n) == EDHIP_ERR_INVALID && said("invalid axis list"));
    CHECK(check_naxis(-3, nullptr, 0) == EDHIP_ERR_INVALID);
    CHECK(check_naxis(8, msg, n) == EDHIP_ERR_UNSUPPORTED && said("more than 7 deformed axes are not supported on the GPU"));
    CHECK(check_naxis(1, msg, n) == EDHIP_OK && check_naxis(7, msg, n) == EDHIP_OK);

    // ---- check_displacement ------------------------------------------------------------------------------------
    int64_t points = -1;
    CHECK(check_displacement(nullptr, 2, &points, msg, n) == EDHIP_ERR_INVALID && said("invalid displacement shape"));
    CHECK(check_displacement(desc(0, {}).get(), 2, nullptr, msg, n) == EDHIP_ERR_INVALID);
    CHECK(check_displacement(desc(9, {2, 2, 2, 2, 2, 2, 2, 2}).get(), 8, nullptr, msg, n) == EDHIP_ERR_INVALID);
    CHECK(check_displacement(desc(9, {8, 2, 2, 2, 2, 2, 2, 2}).get(), 7, nullptr, msg, n) == EDHIP_ERR_INVALID);
    CHECK(check_displacement(desc(3, {3, 3, 3}).get(), 2, nullptr, msg, n) == EDHIP_ERR_INVALID);
    CHECK(check_displacement(desc(3, {2, 3, 3}, 13).get(), 2, nullptr, msg, n) == EDHIP_ERR_DTYPE && said("data type not supported"));
    CHECK(check_displacement(desc(3, {2, 3, 3}, -1).get(), 2, nullptr, msg, n) == EDHIP_ERR_DTYPE);
    CHECK(check_displacement(desc(3, {2, 0, 3}, 13).get(), 2, nullptr, msg, n) == EDHIP_ERR_DTYPE);     // dtype before extents
    CHECK(check_displacement(desc(3, {2, 0, 3}).get(), 2, nullptr, msg, n) == EDHIP_ERR_INVALID);
    CHECK(check_displacement(desc(3, {2, 3, -3}).get(), 2, &points, msg, n) == EDHIP_ERR_INVALID && points == -1);
    CHECK(check_displacement(desc(1, {0}).get(), 0, nullptr, msg, n) == EDHIP_ERR_INVALID);            // naxis 0: shape[0] == 0 is an empty axis
    CHECK(check_displacement(desc(3, {2, 3, 5}, EDHIP_F64).get(), 2, &points, msg, n) == EDHIP_OK && points == 30);
    CHECK(check_displacement(desc(8, {7, 1, 1, 1, 1, 1, 1, 1}).get(), 7, &points, nullptr, 0) == EDHIP_OK && points == 7);

    // ---- check_pairs -------------------------------------------------------------------------------------------
    {
        auto x = desc(2, {8, 9});
        std::vector<int32_t> axis{0, 1}, one{3}, mode{4};
        std::unique_ptr<int32_t[]> none(new int32_t[0]);           // an axis list of no elements: any read is out of bounds
        std::vector<double> cval{0.0};
        auto pairs = [&](const edhip_array* in, const edhip_array* out, int nin, int naxis, const int32_t* ax,
                         int order = 3, int md = 4, bool float_only = false) {
            one[0] = order;
            mode[0] = md;
            return check_pairs(in, out, nin, naxis, ax, one.data(), mode.data(), cval.data(), float_only, msg, n);
        };
        CHECK(pairs(x.get(), x.get(), 1, 2, axis.data()) == EDHIP_OK);
        CHECK(pairs(nullptr, x.get(), 1, 2, axis.data()) == EDHIP_ERR_INVALID && said("invalid number of inputs/outputs"));
        CHECK(pairs(x.get(), x.get(), 0, 2, axis.data()) == EDHIP_ERR_INVALID);
        CHECK(pairs(x.get(), x.get(), EDHIP_MAX_INPUTS + 1, 2, axis.data()) == EDHIP_ERR_INVALID);
        CHECK(check_pairs(x.get(), x.get(), 1, 2, nullptr, one.data(), mode.data(), cval.data(), false, msg, n) == EDHIP_ERR_INVALID &&
              said("invalid axis list"));
        CHECK(check_pairs(x.get(), x.get(), 1, 2, axis.data(), one.data(), mode.data(), nullptr, false, msg, n) == EDHIP_ERR_INVALID);
        CHECK(pairs(x.get(), x.get(), 1, 0, none.get()) == EDHIP_ERR_INVALID && said("invalid axis list"));          // an empty axis list is not read
        CHECK(pairs(x.get(), x.get(), 1, 8, none.get()) == EDHIP_ERR_UNSUPPORTED);
        CHECK(pairs(desc(0, {}).get(), desc(0, {}).get(), 1, 2, axis.data()) == EDHIP_ERR_UNSUPPORTED && said("arrays must have 1..8 dimensions"));
        CHECK(pairs(desc(9, {2, 2, 2, 2, 2, 2, 2, 2}).get(), desc(9, {2, 2, 2, 2, 2, 2, 2, 2}).get(), 1, 2, axis.data()) == EDHIP_ERR_UNSUPPORTED);
        CHECK(pairs(desc(9, {2, 2}).get(), x.get(), 1, 2, axis.data()) == EDHIP_ERR_INVALID && said("input and output dimensions should match"));
        CHECK(pairs(desc(2, {8, 9}, 13).get(), x.get(), 1, 2, axis.data()) == EDHIP_ERR_DTYPE);
        CHECK(pairs(desc(2, {8, 9}, EDHIP_I16).get(), x.get(), 1, 2, axis.data()) == EDHIP_OK);
        CHECK(pairs(desc(2, {8, 9}, EDHIP_I16).get(), x.get(), 1, 2, axis.data(), 3, 4, true) == EDHIP_ERR_DTYPE);
        CHECK(pairs(x.get(), desc(2, {8, 9}, EDHIP_F16).get(), 1, 2, axis.data(), 3, 4, true) == EDHIP_ERR_DTYPE);
        CHECK(pairs(x.get(), x.get(), 1, 2, std::vector<int32_t>{0, 2}.data()) == EDHIP_ERR_INVALID && said("invalid axis in axis list"));
        CHECK(pairs(x.get(), x.get(), 1, 2, std::vector<int32_t>{-1, 1}.data(), 6) == EDHIP_ERR_INVALID && said("invalid axis in axis list"));
        CHECK(pairs(x.get(), x.get(), 1, 2, axis.data(), 6, 9) == EDHIP_ERR_INVALID && said("spline order not supported"));
        CHECK(pairs(x.get(), x.get(), 1, 2, axis.data(), 5, -1) == EDHIP_ERR_INVALID && said("boundary mode not supported"));
        CHECK(pairs(desc(2, {-8, 9}).get(), desc(2, {-8, 9}).get(), 1, 2, axis.data()) == EDHIP_OK);                    // extents are the geometry's business
        // two pairs: the second against the first
        std::unique_ptr<edhip_array[]> ins(new edhip_array[2]), outs(new edhip_array[2]);
        ins[0] = outs[0] = outs[1] = *x;
        ins[1] = *desc(2, {8, 10});
        std::vector<int32_t> axis2{0, 1, 0, 1}, two{3, 3}, modes2{4, 4};
        std::vector<double> cvals2{0.0, 0.0};
        CHECK(check_pairs(ins.get(), outs.get(), 2, 2, axis2.data(), two.data(), modes2.data(), cvals2.data(), false, msg, n) ==
                  EDHIP_ERR_INVALID && said("all inputs should have the same size"));
        ins[1] = *x;
        outs[1] = *desc(2, {7, 9});
        CHECK(check_pairs(ins.get(), outs.get(), 2, 2, axis2.data(), two.data(), modes2.data(), cvals2.data(), false, msg, n) ==
                  EDHIP_ERR_INVALID && said("all outputs should have the same size"));
    }

    // ---- deformed_lengths, sample ------------------------------------------------------------------------------
    {
        auto in = desc(3, {4, 8, 9}), out = desc(3, {4, 6, 7});
        std::vector<int32_t> axis{2, 1};
        std::vector<int64_t> il(2), ol(2);
        deformed_lengths(*in, *out, 2, axis.data(), il.data(), ol.data());
        CHECK(il[0] == 9 && il[1] == 8 && ol[0] == 7 && ol[1] == 6);
        deformed_lengths(*in, *out, 0, nullptr, nullptr, nullptr);
        const edhip_array s = sample(*in, 3, -256);
        CHECK((char*)s.data == (char*)in->data - 768 && s.ndim == 3 && s.shape[2] == 9 && s.stride_bytes[0] == in->stride_bytes[0]);
        CHECK(sample(*in, 0, (int64_t)1 << 40).data == in->data);
    }

    // ---- fill_geometry -----------------------------------------------------------------------------------------
    {
        auto d = desc(3, {2, 3, 5}, EDHIP_F64);
        std::vector<int64_t> il{8, 9}, ol{6, 7}, off{1, 2};
        std::vector<double> aff{1, 0, 0, 0, 1, 0};
        std::unique_ptr<GridGeom> g(new GridGeom);
        CHECK(fill_geometry(d.get(), il.data(), ol.data(), nullptr, 2, nullptr, *g, msg, n) == EDHIP_OK);
        CHECK(g->naxis == 2 && !g->has_affine && g->nvox == 42 && g->ncp[0] == 3 && g->ncp[1] == 5 && g->off[0] == 0 && g->off[1] == 0);
        CHECK(g->disp == (const char*)d->data && g->disp_stride[0] == d->stride_bytes[0] && g->disp_stride[2] == 8);
        CHECK(fill_geometry(d.get(), il.data(), ol.data(), off.data(), 2, aff.data(), *g, nullptr, 0) == EDHIP_OK);
        CHECK(g->has_affine && g->off[1] == 2 && g->affine[4] == 1.0 && g->affine[5] == 0.0);
        il[1] = 1;
        CHECK(fill_geometry(d.get(), il.data(), ol.data(), nullptr, 2, nullptr, *g, msg, n) == EDHIP_ERR_INVALID &&
              said("deformed axes must have at least 2 elements"));
        ol[1] = 0;                                             // no output along the short axis: nothing divides by I - 1
        CHECK(fill_geometry(d.get(), il.data(), ol.data(), nullptr, 2, nullptr, *g, msg, n) == EDHIP_OK && g->nvox == 0);
        il[0] = -5;
        CHECK(fill_geometry(d.get(), il.data(), ol.data(), nullptr, 2, nullptr, *g, msg, n) == EDHIP_ERR_INVALID);
        ol[0] = -6;                                            // negative extents: no voxels, no refusal, no launch
        CHECK(fill_geometry(d.get(), il.data(), ol.data(), nullptr, 2, nullptr, *g, msg, n) == EDHIP_OK && g->nvox == 0);
        // seven deformed axes fill every slot of the geometry and not one more
        auto d7 = desc(8, {7, 2, 2, 2, 2, 2, 2, 2}, EDHIP_F32);
        std::vector<int64_t> l7(7, 4);
        std::vector<double> aff7(7 * 8, 0.5);
        CHECK(fill_geometry(d7.get(), l7.data(), l7.data(), l7.data(), 7, aff7.data(), *g, msg, n) == EDHIP_OK);
        CHECK(g->nvox == 16384 && g->ncp[6] == 2 && g->affine[55] == 0.5 && g->disp_stride[7] == 8);
    }
    // ---- the preamble, the axis count of the image-side calls, the flag and the batch limit ----------------------
    strcpy(msg, "stale");
    CHECK(check_batch_call(0, true, msg, n) == EDHIP_OK && said(""));
    CHECK(check_batch_call(-1, true, msg, n) == EDHIP_ERR_INVALID && said("invalid batch"));
    CHECK(check_batch_call(3, false, msg, n) == EDHIP_ERR_INVALID && said("invalid batch"));
    CHECK(check_batch_call(-1, false, nullptr, 0) == EDHIP_ERR_INVALID);
    CHECK(check_batch_call(1, true, msg, 0) == EDHIP_OK && said("invalid batch"));                 // errlen 0: msg is not touched
    {
        std::unique_ptr<int32_t[]> none(new int32_t[0]);           // the list itself is never read
        CHECK(check_axes_1_to_3("f", nullptr, 2, msg, n) == EDHIP_ERR_INVALID && said("invalid axis list"));
        CHECK(check_axes_1_to_3("f", none.get(), 0, msg, n) == EDHIP_ERR_INVALID && said("invalid axis list"));
        CHECK(check_axes_1_to_3("f", none.get(), -7, nullptr, 0) == EDHIP_ERR_INVALID);
        CHECK(check_axes_1_to_3("edhip_f", none.get(), 4, msg, n) == EDHIP_ERR_UNSUPPORTED && said("edhip_f takes 1 to 3 deformed axes"));
        CHECK(check_axes_1_to_3("f", none.get(), 1, msg, n) == EDHIP_OK && check_axes_1_to_3("f", none.get(), 3, msg, n) == EDHIP_OK);
    }
    CHECK(check_prefiltered("edhip_f", EDHIP_FLAG_RAW_DISPLACEMENT | EDHIP_FLAG_FAST, msg, n) == EDHIP_ERR_INVALID &&
          said("edhip_f takes the prefiltered control grid"));
    CHECK(check_prefiltered("edhip_f", EDHIP_FLAG_FAST, msg, n) == EDHIP_OK && check_prefiltered("f", 0, nullptr, 0) == EDHIP_OK);
    CHECK(check_batch_limit("edhip_f", 65536, msg, n) == EDHIP_ERR_UNSUPPORTED && said("edhip_f: too many samples"));
    CHECK(check_batch_limit("f", 65535, msg, n) == EDHIP_OK && check_batch_limit("f", 0, msg, n) == EDHIP_OK);

    // ---- has_shape, f32_or_f64 ---------------------------------------------------------------------------------
    {
        std::vector<int64_t> want{5, 2, 2};
        std::unique_ptr<int64_t[]> none(new int64_t[0]);           // rank 0: no extent is read
        CHECK(has_shape(desc(3, {5, 2, 2}).get(), 3, want.data()) && has_shape(desc(2, {5, 2}).get(), 2, want.data()));
        CHECK(!has_shape(desc(3, {5, 2, 3}).get(), 3, want.data()) && !has_shape(desc(2, {5, 2}).get(), 3, want.data()));
        CHECK(!has_shape(desc(0, {}).get(), 3, want.data()) && !has_shape(desc(9, {5, 2, 2}).get(), 3, want.data()));
        CHECK(!has_shape(desc(-1, {5, 2, 2}).get(), 3, want.data()));
        CHECK(has_shape(desc(0, {}).get(), 0, none.get()) && !has_shape(desc(9, {5, 2, 2}).get(), 0, none.get()));
        CHECK(!has_shape(desc(3, {5, -2, 2}).get(), 3, want.data()));
        want[0] = -5;                                          // a negative extent equals itself: the callers refuse it before
        CHECK(has_shape(desc(3, {-5, 2, 2}).get(), 3, want.data()));
        CHECK(f32_or_f64(desc(1, {4}, EDHIP_F32).get()) && f32_or_f64(desc(0, {}, EDHIP_F64).get()));
        CHECK(!f32_or_f64(desc(1, {4}, EDHIP_F16).get()) && !f32_or_f64(desc(1, {4}, EDHIP_I32).get()));
        CHECK(!f32_or_f64(desc(1, {4}, -1).get()) && !f32_or_f64(desc(9, {4}, 13).get()));
    }

    // ---- check_status ------------------------------------------------------------------------------------------
    CHECK(check_status(nullptr, false, 5, msg, n) == EDHIP_OK && check_status(nullptr, true, -1, nullptr, 0) == EDHIP_OK);
    CHECK(check_status(desc(1, {5}, EDHIP_U8).get(), true, 5, msg, n) == EDHIP_OK);
    CHECK(check_status(desc(1, {0}, EDHIP_U8).get(), true, 0, msg, n) == EDHIP_OK);
    CHECK(check_status(desc(9, {4}, EDHIP_BOOL).get(), false, 5, msg, n) == EDHIP_ERR_INVALID &&
          said("the status belongs to the inverse direction"));                                    // the direction before the array
    CHECK(check_status(desc(1, {4}, EDHIP_BOOL).get(), true, 5, msg, n) == EDHIP_ERR_INVALID && said("status must have shape (N)"));
    CHECK(check_status(desc(0, {}, EDHIP_U8).get(), true, 5, msg, n) == EDHIP_ERR_INVALID);
    CHECK(check_status(desc(9, {5}, EDHIP_U8).get(), true, 5, msg, n) == EDHIP_ERR_INVALID);
    CHECK(check_status(desc(2, {5, 1}, EDHIP_U8).get(), true, 5, msg, n) == EDHIP_ERR_INVALID);
    CHECK(check_status(desc(1, {-5}, EDHIP_U8).get(), true, 5, msg, n) == EDHIP_ERR_INVALID);
    CHECK(check_status(desc(1, {5}, EDHIP_BOOL).get(), true, 5, msg, n) == EDHIP_ERR_DTYPE && said("status must be uint8"));
    CHECK(check_status(desc(1, {5}, -1).get(), true, 5, nullptr, 0) == EDHIP_ERR_DTYPE);

    // ---- check_iteration ---------------------------------------------------------------------------------------
    {
        std::vector<double> aff{1, 0, 0, 0, 1, 0}, lin{1, 0, 0, 1};
        CHECK(check_iteration(1, 1e-300, nullptr, nullptr, msg, n) == EDHIP_OK);
        CHECK(check_iteration(32, 1e-9, aff.data(), lin.data(), msg, n) == EDHIP_OK);
        CHECK(check_iteration(32, 1e-9, nullptr, lin.data(), nullptr, 0) == EDHIP_OK);
        CHECK(check_iteration(0, 0.0, aff.data(), nullptr, msg, n) == EDHIP_ERR_INVALID && said("max_iter must be at least 1"));
        CHECK(check_iteration(-3, 1e-9, nullptr, nullptr, msg, n) == EDHIP_ERR_INVALID);
        CHECK(check_iteration(1, 0.0, aff.data(), nullptr, msg, n) == EDHIP_ERR_INVALID && said("tol must be positive"));
        CHECK(check_iteration(1, -1.0, nullptr, nullptr, msg, n) == EDHIP_ERR_INVALID);
        CHECK(check_iteration(1, std::nan(""), nullptr, nullptr, msg, n) == EDHIP_ERR_INVALID && said("tol must be positive"));
        CHECK(check_iteration(1, 1e-9, aff.data(), nullptr, msg, n) == EDHIP_ERR_INVALID &&
              said("forward_linear is required with an affine map"));
    }

    // ---- batch_array -------------------------------------------------------------------------------------------
    {
        std::unique_ptr<BatchArray> zero(new BatchArray);
        memset(zero.get(), 0, sizeof(BatchArray));
        const BatchArray none = batch_array(nullptr, 4096);        // a null optional array: all zero, the stride too
        CHECK(memcmp(&none, zero.get(), sizeof(BatchArray)) == 0);
        auto a = desc(3, {4, 8, 9}, EDHIP_I16);
        const BatchArray s = batch_array(a.get(), -720);
        CHECK(s.ptr == (char*)a->data && s.dtype == EDHIP_I16 && s.bstride == -720);
        CHECK(s.stride[0] == a->stride_bytes[0] && s.stride[1] == 72 && s.stride[2] == 8 && s.stride[3] == 0 && s.stride[7] == 0);
        a->stride_bytes[5] = 77;                               // beyond the rank: not the array's, not copied
        CHECK(batch_array(a.get(), 0).stride[5] == 0);
        const BatchArray r0 = batch_array(desc(0, {}).get(), 8);
        CHECK(r0.ptr == (char*)0x1000 && r0.stride[0] == 0 && r0.bstride == 8);
        const BatchArray neg = batch_array(desc(-4, {3}).get(), 8);
        CHECK(neg.stride[0] == 0 && neg.bstride == 8);
        auto nine = desc(9, {2, 2, 2, 2, 2, 2, 2, 2});             // rank 9: the eight strides the descriptor has, not a ninth
        const BatchArray r9 = batch_array(nine.get(), 0);
        CHECK(r9.stride[0] == nine->stride_bytes[0] && r9.stride[7] == 8);
        const BatchArray negext = batch_array(desc(2, {-5, 3}).get(), 1);   // extents are not this helper's business
        CHECK(negext.stride[1] == 8 && negext.stride[0] == 24);
    }
    std::printf("ok\n");
    return 0;
}
