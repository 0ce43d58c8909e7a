// shared_defs.hpp -- constants and plain structs that the host headers (class_tables.hpp, side_tables.hpp,
// launch_shapes.hpp, tem_layout.hpp) and the kernels both use.  No HIP: it compiles with any C++17 compiler.
#ifndef TEMX_SHARED_DEFS_HPP
#define TEMX_SHARED_DEFS_HPP

namespace temx {

// ---- row table of the latitude-class sweeps (kernels_cls.hpp; built by class_tables.hpp) -------------------------
constexpr int CLS_MB = 4;                     // member rows per class and batch
constexpr int CLS_PADB = 10;                  // batches of padding behind crow (index loads run up to PD + 1 ahead)
constexpr int CLS_HASPAD_BIT = 1 << 27;       // the batch has at least one padding entry (set in all its entries)
constexpr int CLS_SOUTH = 1, CLS_FIRST = 2, CLS_LAST = 4;   // flags, stored at bit 28

// ---- mirror-paired sweeps (kernels_sym.hpp; cut by tem_layout.hpp) ------------------------------------------------
constexpr int SYM_PROJ_CH = 3;                // pair-groups per chunk of the paired project sweep

// ---- vertical interpolation (kernels_vert.hpp; shape chosen by launch_shapes.hpp, vert_slab_shape) ---------------
constexpr int VERT_THREADS = 256;

// LDS of a workgroup of vert_slab_kernel: [int bad[VERT_THREADS]] [fp64 P image, field mode] [NF input images]
// [NF output images]; every image starts on a 16-byte boundary.
struct VertSlab {
  int cw;        // columns per workgroup
  int nseg;      // walks (lanes) per (column, time)
  int seg;       // brackets per walk
  int in_stride, out_stride;   // elements per column in the LDS images (odd)
  int in_img, out_img, p_img;  // bytes per image
};

// ---- re-layout (kernels_layout.hpp): tile of a launch, chosen by launch_shapes.hpp, layout_tile ------------------
struct LayoutTile {
  int tc_shift;   // TC = 1 << tc_shift columns, 32 or 64
  int kl;         // destination levels per tile
  int tt;         // times per tile (== ntb unless kl == 1)
  int stride;     // LDS elements per column, odd, >= kl * tt
  int nct, nlt, ntt;   // tiles along ncol, nlev, ntb
};

// ---- fused ingestion (kernels_ingest.hpp): tile of a launch, chosen by launch_shapes.hpp, ingest_tile -------------
constexpr int INGEST_THREADS = 256;
constexpr int INGEST_LDS_BYTES = 48 * 1024;   // per workgroup: three workgroups per CU, one loads while another walks

// LDS of a workgroup of ingest_kernel: [fp64 ps image] [nf fields][kw + 1 level slots] images of the destination dtype;
// an image is TC columns of `stride` elements.
struct IngestTile {
  int tc_shift;   // TC = 1 << tc_shift columns, 16 .. 256
  int tt;         // times per tile
  int kw;         // brackets per level window: a window holds kw + 1 levels, its first the last of the one before
  int stride;     // LDS elements per column, odd, >= tt
  int ppl;        // (column, time) pairs per lane: ceil(TC * tt / INGEST_THREADS)
  int nct, ntt;   // tiles along ncol, ntb
  int nwin;       // level windows: ceil((nlev - 1) / kw)
};

}  // namespace temx

#endif
