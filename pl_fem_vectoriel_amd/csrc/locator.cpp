// Host half of the point locator (symbolic.h, loc_*): a uniform cell grid over the vertex bounding box with a CSR list
// from every cell to the elements whose bounding box touches it.  Built on first request (plfem_locator_*,
// plfem_symbolic_get("loc_*")), never by the analysis itself: the cold-solve path does not pay for it.
#include <algorithm>
#include <chrono>
#include <cmath>

#include "symbolic.h"

namespace plfem {

namespace {
inline int cell_of(double v, double v0, double inv_h, int n) {
  const double f = std::floor((v - v0) * inv_h);
  if (!(f >= 0.0)) return 0;                   // (also NaN)
  return f >= (double)(n - 1) ? n - 1 : (int)f;
}
}  // namespace

void ensure_locator(const Symbolic& S) {
  if (!S.loc_cell_ptr.empty()) return;
  const auto t0 = std::chrono::steady_clock::now();
  const int ne = S.ne, N = S.N, nv = S.nv;
  const double* px = S.doflocs.data();         // the first nv DOFs are the vertices
  const double* py = S.doflocs.data() + N;
  double xmin = px[0], xmax = px[0], ymin = py[0], ymax = py[0];
  for (int v = 1; v < nv; ++v) {
    xmin = std::min(xmin, px[v]); xmax = std::max(xmax, px[v]);
    ymin = std::min(ymin, py[v]); ymax = std::max(ymax, py[v]);
  }
  const double w = xmax > xmin ? xmax - xmin : 1.0, h = ymax > ymin ? ymax - ymin : 1.0;
  // about LOC_CELLS_PER_ELEM cells per element, square cells, never more than that many in all
  const int64_t target = (int64_t)LOC_CELLS_PER_ELEM * ne;
  int nx = (int)std::max<int64_t>(1, std::min<int64_t>(target, (int64_t)std::floor(std::sqrt((double)target * w / h))));
  int ny = (int)std::max<int64_t>(1, target / nx);
  const double inv_hx = nx / w, inv_hy = ny / h;
  S.loc_grid = {xmin, ymin, inv_hx, inv_hy, (double)nx, (double)ny};
  const int64_t ncell = (int64_t)nx * ny;
  const int32_t* t = S.tsorted.data();
  auto bbox_cells = [&](int e, int& ix0, int& ix1, int& iy0, int& iy1) {
    const int32_t a = t[e], b = t[(size_t)ne + e], c = t[2 * (size_t)ne + e];
    ix0 = cell_of(std::min(px[a], std::min(px[b], px[c])), xmin, inv_hx, nx);
    ix1 = cell_of(std::max(px[a], std::max(px[b], px[c])), xmin, inv_hx, nx);
    iy0 = cell_of(std::min(py[a], std::min(py[b], py[c])), ymin, inv_hy, ny);
    iy1 = cell_of(std::max(py[a], std::max(py[b], py[c])), ymin, inv_hy, ny);
  };
  std::vector<int32_t> cnt(ncell + 1, 0);
  for (int e = 0; e < ne; ++e) {
    int ix0, ix1, iy0, iy1;
    bbox_cells(e, ix0, ix1, iy0, iy1);
    for (int iy = iy0; iy <= iy1; ++iy)
      for (int ix = ix0; ix <= ix1; ++ix) ++cnt[(size_t)iy * nx + ix + 1];
  }
  int32_t maxc = 0;
  for (int64_t i = 0; i < ncell; ++i) {
    maxc = std::max(maxc, cnt[i + 1]);
    cnt[i + 1] += cnt[i];
  }
  std::vector<int32_t> elems(cnt[ncell]);
  std::vector<int32_t> fill(cnt.begin(), cnt.end() - 1);
  for (int e = 0; e < ne; ++e) {                // ascending e: every cell's list comes out sorted
    int ix0, ix1, iy0, iy1;
    bbox_cells(e, ix0, ix1, iy0, iy1);
    for (int iy = iy0; iy <= iy1; ++iy)
      for (int ix = ix0; ix <= ix1; ++ix) elems[fill[(size_t)iy * nx + ix]++] = e;
  }
  const double secs = std::chrono::duration<double>(std::chrono::steady_clock::now() - t0).count();
  S.loc_stats = {(double)ncell, (double)cnt[ncell] / (double)ncell, (double)maxc, secs};
  S.loc_cell_elems.swap(elems);
  S.loc_cell_ptr.swap(cnt);
}

// An edge node has one adjacent element (outer boundary) or two (the analysis rejects a non-manifold mesh): the neighbour
// across the edge is the one that is not the element itself.
void ensure_elem_nbr(const Symbolic& S) {
  if (!S.elem_nbr.empty()) return;
  const int ne = S.ne;
  std::vector<int32_t> nbr((size_t)3 * ne, -1);
  for (int l = 0; l < 3; ++l)
    for (int e = 0; e < ne; ++e) {
      const int32_t node = S.edof[(size_t)(3 + l) * ne + e];
      for (int32_t q = S.nptr[node]; q < S.nptr[node + 1]; ++q)
        if (S.nadj[q] != e) nbr[(size_t)l * ne + e] = S.nadj[q];
    }
  S.elem_nbr.swap(nbr);
}

}  // namespace plfem
