"""Periodic k-nearest-neighbour bond graphs built on the device.

The reference builds the bond graph on the CPU, per structure, with jarvis' neighbour lists
(``alignn/graphs.py:155-264``: ``nearest_neighbor_edges`` + ``build_undirected_edgedata``) - and the ASE calculators
rebuild it at EVERY molecular-dynamics step (``alignn/ff/calculators.py:280-291``).  With the model's energies + forces
at 14 ms for 3 200 atoms (fused eval path) that host-side build is what bounds MD.  This module restates the same
construction as device tensor operations, so positions never leave the GPU:

* all periodic images within ``cutoff`` and farther than jarvis' ``bond_tol`` = 0.15 A (enough images along each lattice
  vector: cutoff / plane spacing - for fractional coordinates in [0, 1]; for UNWRAPPED coordinates the box jarvis lays out
  around the fractional extent, ``_image_box``: once the fractions span more than a cell that box misses images inside
  the cutoff, and the reference's bond list - reproduced here - is defined by what it scans, not by the geometry);
* too few neighbours somewhere -> widen the search sphere (``graphs.py:170-188``);
* per site keep everything out to the shell of the ``max_neighbors``-th neighbour (ties with it included);
* canonise to an undirected multigraph keyed (smaller id, larger id, image) and emit both directions as a consecutive
  pair with ``r`` = Cartesian displacement src -> dst (``graphs.py:128-153, 230-264, 550``).

It is the same algorithm (and gives the same edge list, in the same order) as ``alignn_amd.synthetic.knn_multigraph``,
the numpy restatement every test input of this repository comes from; distances are evaluated in float64 so that the
shell / tie decisions are identical.  ``knn_multigraph`` / ``knn_multigraph_batch`` are plain torch tensor operations
(broadcast distance, sort, unique: any device, the CPU twin and the checker); ``knn_multigraph_batch_hip`` is the same
construction on the hand-written kernels of ``csrc/knn.hip`` (one wavefront per site, no padded [B,n,n,I] tensors, one
host read per batch) and is what ``crystal_batch`` uses on the GPU.

``crystal_batch`` chains it with ``graph.build_csr`` / ``graph.line_graph_of``: positions -> canonical ``GraphBatch``
without a host round trip of any per-bond array.
"""

from __future__ import annotations

from typing import Optional, Sequence

import torch

from .graph import GraphBatch, _ptr_from_counts, build_csr, csr_and_line_graph, line_graph_of

__all__ = ["knn_multigraph", "knn_multigraph_batch", "knn_multigraph_batch_hip", "radius_graph", "radius_graph_batch",
           "radius_graph_batch_hip", "crystal_batch", "clear_lattice_cache"]

PAD_BUDGET = 2 << 30  # bytes of padded distance tensor above which knn_multigraph_batch goes crystal by crystal


BOND_TOL = 0.15  # jarvis' get_all_neighbors(r, bond_tol=0.15): anything closer than this is not a neighbour


def _image_box(spacing: torch.Tensor, fmin: torch.Tensor, fmax: torch.Tensor, cut: torch.Tensor):
    """Inclusive image range ``(lo, hi)`` (float64, integer valued) a crystal scans at cutoff ``cut`` - the rule of
    ``alignn_amd.synthetic.image_box``.  Axis with all fractions inside [0, 1]: ``|I| <= ceil(cut / plane spacing)``,
    every image within the cutoff.  Otherwise the box jarvis lays out: ``floor(min frac) - maxr .. ceil(max frac) + maxr
    - 1``, ``maxr = ceil((cut + BOND_TOL) / spacing)``.  ``spacing``, ``fmin``, ``fmax`` [..., 3]; ``cut`` broadcastable to
    them."""
    reach = torch.ceil(cut / spacing)
    maxr = torch.ceil((cut + BOND_TOL) / spacing)
    flo, fhi = torch.floor(fmin), torch.ceil(fmax)
    wrapped = (flo == 0) & (fhi <= 1)
    return torch.where(wrapped, -reach, flo - maxr), torch.where(wrapped, reach, fhi + maxr - 1)


def _all_neighbors(lat: torch.Tensor, frac: torch.Tensor, cutoff: float):
    inv = torch.linalg.inv(lat)
    spacing = 1.0 / torch.linalg.norm(inv, dim=0)
    lo, hi = _image_box(spacing, frac.min(dim=0).values, frac.max(dim=0).values, torch.as_tensor(cutoff, dtype=lat.dtype, device=lat.device))
    box = torch.stack([lo, hi]).to(torch.int64).tolist()  # 6 small integers (host)
    rng = [torch.arange(a, b + 1, device=lat.device) for a, b in zip(*box)]
    images = torch.stack(torch.meshgrid(*rng, indexing="ij"), -1).reshape(-1, 3)
    # explicit elementwise float64 operations in the same fixed order as alignn_amd.synthetic._all_neighbors (separate
    # multiply / add kernels, no matmul, no fused multiply-add): identical distance bits, identical tie decisions
    cart = frac[:, 0:1] * lat[0] + frac[:, 1:2] * lat[1] + frac[:, 2:3] * lat[2]
    imf = images.to(lat.dtype)
    shift = imf[:, 0:1] * lat[0] + imf[:, 1:2] * lat[1] + imf[:, 2:3] * lat[2]
    d = (cart[None, :, None, :] + shift[None, None, :, :]) - cart[:, None, None, :]  # d[i, j, I] = cart[j] + shift[I] - cart[i]
    dx, dy, dz = d[..., 0], d[..., 1], d[..., 2]
    dist = torch.sqrt(dx * dx + dy * dy + dz * dz)
    src, dst, img = torch.nonzero((dist <= cutoff) & (dist > BOND_TOL), as_tuple=True)
    return src, dst, images[img], dist[src, dst, img]


def knn_multigraph(lat, frac, cutoff: float = 8.0, max_neighbors: int = 12, device=None):
    """``lat`` [3,3] (rows a, b, c), ``frac`` [n,3] fractional coordinates -> ``(u, v, r)``: int64 [E], int64 [E],
    float32 [E,3] on ``device`` (default: where ``frac`` lives), both directions of every bond stored consecutively."""
    frac = torch.as_tensor(frac)
    dev = torch.device(device) if device is not None else frac.device
    lat = torch.as_tensor(lat).to(dev, torch.float64)
    frac = frac.to(dev, torch.float64)
    n = frac.shape[0]
    k = max_neighbors
    while True:
        src, dst, img, dist = _all_neighbors(lat, frac, cutoff)
        counts = torch.bincount(src, minlength=n)
        if int(counts.min()) >= k:
            break
        longest = float(torch.linalg.norm(lat, dim=1).max())
        cutoff = longest if cutoff < longest else 2.0 * cutoff
    # per site: everything out to the shell of the k-th neighbour (lexsort by (src, dist) as two stable sorts)
    o = torch.argsort(dist, stable=True)
    o = o[torch.argsort(src[o], stable=True)]
    src, dst, img, dist = src[o], dst[o], img[o], dist[o]
    first = torch.cumsum(counts, 0) - counts
    kth = dist[first + k - 1]
    keep = dist <= kth[src]
    src, dst, img = src[keep], dst[keep], img[keep]
    # canonical key: smaller id first, image measured from the first vertex; set semantics, sorted order
    swap = dst < src
    a = torch.where(swap, dst, src)
    b = torch.where(swap, src, dst)
    im = torch.where(swap[:, None], -img, img)
    key = torch.unique(torch.cat([a[:, None], b[:, None], im], 1), dim=0)
    a, b, im = key[:, 0], key[:, 1], key[:, 2:5]
    d = (frac[b] + im.to(frac.dtype) - frac[a]) @ lat
    u = torch.stack([a, b], 1).reshape(-1)
    v = torch.stack([b, a], 1).reshape(-1)
    r = torch.stack([d, -d], 1).reshape(-1, 3).to(torch.float32)
    return u, v, r


def knn_multigraph_batch(lattices: Sequence, fracs: Sequence, cutoff: float = 8.0, max_neighbors: int = 12, device=None):
    """``knn_multigraph`` for a whole batch of crystals at once: -> ``(u, v, r, num_nodes)`` with the bonds of crystal
    0, 1, ... concatenated (atom ids offset): the same bond list in the same order as running ``knn_multigraph`` per
    crystal and concatenating (index arrays equal, bond vectors equal to the last bit or two).  The crystals are padded to a common atom count and share one image grid (the largest
    reach of the batch), so the host is consulted twice per BATCH (that reach; "does any site still lack neighbours")
    instead of twice per crystal."""
    dev = torch.device(device) if device is not None else torch.as_tensor(fracs[0]).device
    B = len(fracs)
    ns = [int(torch.as_tensor(f).shape[0]) for f in fracs]
    nmax = max(ns)
    lat = torch.stack([torch.as_tensor(x).to(dev, torch.float64) for x in lattices])  # [B,3,3]
    # The padded form materialises float64 [B, nmax, nmax, I, 3] for the LARGEST image grid of the batch: a 2-atom cell that
    # needs 729 images next to a 100-atom cell makes that tens of GB where each crystal alone needs MBs.  Estimate both
    # volumes from the lattices (no host read of device data beyond the 9 x B lattice entries the caller passed in) and
    # take the per-crystal loop when padding would cost more than PAD_BUDGET bytes or 8x the ragged volume.
    if B > 1:
        lat_h = lat.detach().cpu()
        sp = 1.0 / torch.linalg.norm(torch.linalg.inv(lat_h), dim=1)
        reach_h = torch.ceil(float(cutoff) / sp).to(torch.int64)
        imgs = (2 * reach_h + 1).prod(dim=1)
        padded = B * nmax * nmax * int((2 * reach_h.max(dim=0).values + 1).prod()) * 3 * 8
        ragged = int(sum(n * n * int(i) for n, i in zip(ns, imgs.tolist()))) * 3 * 8
        if padded > PAD_BUDGET or padded > 8 * max(ragged, 1):
            us, vs, rs, off = [], [], [], 0
            for b in range(B):
                u, v, r = knn_multigraph(lat[b], torch.as_tensor(fracs[b]), cutoff, max_neighbors, device=dev)
                us.append(u + off)
                vs.append(v + off)
                rs.append(r)
                off += ns[b]
            return torch.cat(us), torch.cat(vs), torch.cat(rs), ns
    frac = torch.zeros(B, nmax, 3, dtype=torch.float64, device=dev)
    for b, f in enumerate(fracs):
        frac[b, :ns[b]] = torch.as_tensor(f).to(dev, torch.float64)
    n_t = torch.tensor(ns, device=dev)
    real = torch.arange(nmax, device=dev)[None, :] < n_t[:, None]  # [B,nmax]
    k = max_neighbors
    cut = torch.full((B,), float(cutoff), dtype=torch.float64, device=dev)
    longest = torch.linalg.norm(lat, dim=2).max(dim=1).values
    spacing = 1.0 / torch.linalg.norm(torch.linalg.inv(lat), dim=1)  # [B,3]: plane spacings (column norms of the inverse)
    # same fixed-order float64 arithmetic as knn_multigraph / synthetic._all_neighbors
    cart = frac[..., 0:1] * lat[:, None, 0, :] + frac[..., 1:2] * lat[:, None, 1, :] + frac[..., 2:3] * lat[:, None, 2, :]
    pad = ~real[:, :, None]
    fmin = frac.masked_fill(pad, float("inf")).min(dim=1).values  # [B,3] fractional extent of the real sites
    fmax = frac.masked_fill(pad, float("-inf")).max(dim=1).values
    while True:
        lo, hi = (x.to(torch.int64) for x in _image_box(spacing, fmin, fmax, cut[:, None]))  # [B,3] each
        box = torch.stack([lo.min(dim=0).values, hi.max(dim=0).values]).tolist()  # host: six integers per batch
        rng = [torch.arange(a, b + 1, device=dev) for a, b in zip(*box)]
        images = torch.stack(torch.meshgrid(*rng, indexing="ij"), -1).reshape(-1, 3)  # [I,3]
        inside = ((images[None, :, :] >= lo[:, None, :]) & (images[None, :, :] <= hi[:, None, :])).all(-1)  # [B,I]: the images crystal b itself would scan
        imf = images.to(torch.float64)
        shift = imf[None, :, 0:1] * lat[:, None, 0, :] + imf[None, :, 1:2] * lat[:, None, 1, :] + imf[None, :, 2:3] * lat[:, None, 2, :]
        d = (cart[:, None, :, None, :] + shift[:, None, None, :, :]) - cart[:, :, None, None, :]  # [B,i,j,I,3]
        dx, dy, dz = d[..., 0], d[..., 1], d[..., 2]
        dist = torch.sqrt(dx * dx + dy * dy + dz * dz)
        ok = ((dist <= cut[:, None, None, None]) & (dist > BOND_TOL) & real[:, :, None, None] & real[:, None, :, None]
              & inside[:, None, None, :])
        counts = ok.sum(dim=(2, 3))  # [B,nmax] neighbours per site
        short = ((counts < k) & real).any(dim=1)  # [B]
        if not bool(short.any()):  # host: one flag per batch
            break
        cut = torch.where(short, torch.where(cut < longest, longest, 2.0 * cut), cut)
    # per site: everything out to the shell of the k-th neighbour
    dm = torch.where(ok, dist, torch.full_like(dist, float("inf"))).reshape(B, nmax, -1)
    kth = torch.sort(dm, dim=2).values[:, :, k - 1]  # [B,nmax]
    keep = ok & (dist <= kth[:, :, None, None])
    b_i, src, dst, img = torch.nonzero(keep, as_tuple=True)
    im = images[img]
    swap = dst < src
    a_ = torch.where(swap, dst, src)
    c_ = torch.where(swap, src, dst)
    im = torch.where(swap[:, None], -im, im)
    key = torch.unique(torch.cat([b_i[:, None], a_[:, None], c_[:, None], im], 1), dim=0)  # sorted by (crystal, a, b, image)
    kb, a_, c_, im = key[:, 0], key[:, 1], key[:, 2], key[:, 3:6]
    disp = (frac[kb, c_] + im.to(torch.float64) - frac[kb, a_])
    dvec = torch.bmm(disp.unsqueeze(1), lat[kb]).squeeze(1)
    off = (torch.cumsum(n_t, 0) - n_t)[kb]
    u = torch.stack([a_ + off, c_ + off], 1).reshape(-1)
    v = torch.stack([c_ + off, a_ + off], 1).reshape(-1)
    r = torch.stack([dvec, -dvec], 1).reshape(-1, 3).to(torch.float32)
    return u, v, r, ns


# ---------------------------------------------------------------------------------------------------------------------
# radius graphs (alignn/graphs.py:267-364) - what the reference's force-field configs select (neighbor_strategy
# "radius_graph", alignn/examples/sample_data_ff/config_example_atomwise.json:6,37: cutoff 4.0)
# ---------------------------------------------------------------------------------------------------------------------
RADIUS_LEVELS = 24  # cutoff, cutoff + 0.5, ... tried per crystal (the reference loops without a bound)


def _radius_box(lat64: torch.Tensor, frac32: torch.Tensor, cutoff: float, bond_tol: float):
    """Image box [nmin, nmax) per axis as the reference lays it out (graphs.py:296-309): floor / ceil of the fractional
    extent, widened by maxr = ceil((cutoff + bond_tol) / plane spacing) - evaluated in float64 with a hair of slack: a box
    larger than needed changes neither the edge set (every image within the cutoff is inside either way) nor the edge
    order (lexicographic in the image index)."""
    spacing = 1.0 / torch.linalg.norm(torch.linalg.inv(lat64), dim=0)
    maxr = torch.ceil((cutoff + bond_tol) / spacing + 1e-9)
    nmin = torch.floor(frac32.min(dim=0).values.double()) - maxr
    nmax = torch.ceil(frac32.max(dim=0).values.double()) + maxr
    return nmin.to(torch.int64), nmax.to(torch.int64)


def _radius_pass(lat32, cart32, nmin, nmax, cutoff: float, atol: float):
    """One ``temp_graph`` of the reference (graphs.py:278-346) in float32, every operation spelled out (separate multiplies
    and adds in a fixed order - the HIP kernel csrc/radius.hip evaluates the same sequence)."""
    dev = lat32.device
    rng = [torch.arange(int(a), int(b), device=dev) for a, b in zip(nmin.tolist(), nmax.tolist())]
    images = torch.stack(torch.meshgrid(*rng, indexing="ij"), -1).reshape(-1, 3)  # cartesian_prod order: i0 major
    imf = images.to(torch.float32)
    shift = (imf[:, 0:1] * lat32[0] + imf[:, 1:2] * lat32[1]) + imf[:, 2:3] * lat32[2]  # [I,3]
    x_dst = shift[:, None, :] + cart32[None, :, :]  # [I,n,3]; flat index = image * n + atom (graphs.py:314-318)
    d = cart32[:, None, None, :] - x_dst[None]  # [n,I,n,3]
    dx, dy, dz = d[..., 0], d[..., 1], d[..., 2]
    dist = torch.sqrt((dx * dx + dy * dy) + dz * dz)
    keep = (dist <= cutoff) & ~(dist <= atol)  # isclose(dist, 0, atol) with rtol * 0 = 0
    u, img, v = torch.nonzero(keep, as_tuple=True)  # torch.where order: by source, then image, then destination atom
    r = x_dst[img, v] - cart32[u]
    return u, v, r, images[img]


def radius_graph(lat, frac, cutoff: float = 5.0, bond_tol: float = 0.5, atol: float = 1e-5, cutoff_extra: float = 0.5,
                 device=None, return_cutoff: bool = False):
    """The reference's ``radius_graph`` (alignn/graphs.py:267-364) as tensor operations on any device: all pairs (site,
    periodic image of a site) with ``atol < distance <= cutoff`` in ``torch.where`` order (by source atom, then image, then
    destination atom - the two directions of a bond are NOT adjacent), the cutoff widened by ``cutoff_extra`` until the
    last site appears in the graph (``dgl.graph((u, v)).num_nodes() == n``: the reference's stopping rule).
    ``lat`` [3,3] (rows a, b, c), ``frac`` [n,3] -> ``(u, v, r, images)``: int64 [E] x 2, float32 [E,3], int64 [E,3].
    float32 distances, as in the reference (``torch.get_default_dtype()``); this is the CPU twin and the checker of
    ``radius_graph_batch_hip`` (bit-identical arrays)."""
    frac = torch.as_tensor(frac)
    dev = torch.device(device) if device is not None else frac.device
    lat64 = torch.as_tensor(lat).to(dev, torch.float64)
    frac64 = frac.to(dev, torch.float64)
    n = frac64.shape[0]
    cart64 = frac64[:, 0:1] * lat64[0] + frac64[:, 1:2] * lat64[1] + frac64[:, 2:3] * lat64[2]  # (jarvis: float64 product)
    lat32, cart32, frac32 = lat64.float(), cart64.float(), frac64.float()
    c = float(cutoff)
    for _ in range(RADIUS_LEVELS):
        nmin, nmax = _radius_box(lat64, frac32, c, bond_tol)
        u, v, r, images = _radius_pass(lat32, cart32, nmin, nmax, c, atol)
        if u.numel() and int(torch.maximum(u.max(), v.max())) + 1 == n:
            return (u, v, r, images, c) if return_cutoff else (u, v, r, images)
        c += cutoff_extra
    raise RuntimeError(f"radius_graph: the last site has no neighbour within {c} A")


def radius_graph_batch(lattices: Sequence, fracs: Sequence, cutoff: float = 5.0, device=None, return_images: bool = False):
    """Crystal by crystal through ``radius_graph`` with atom ids offset per crystal -> ``(u, v, r, num_atoms)`` like
    ``knn_multigraph_batch`` (any device: the CPU path of ``crystal_batch(neighbor_strategy="radius_graph")``)."""
    us, vs, rs, ims, ns, off = [], [], [], [], [], 0
    for lat, frac in zip(lattices, fracs):
        u, v, r, im = radius_graph(lat, frac, cutoff, device=device)
        us.append(u + off), vs.append(v + off), rs.append(r), ims.append(im)
        ns.append(int(torch.as_tensor(frac).shape[0]))
        off += ns[-1]
    out = (torch.cat(us), torch.cat(vs), torch.cat(rs), ns)
    return out + ((torch.cat(ims).to(torch.int32),) if return_images else ())


def radius_graph_batch_hip(lattices: Sequence, fracs: Sequence, cutoff: float = 5.0, bond_tol: float = 0.5, atol: float = 1e-5,
                           cutoff_extra: float = 0.5, device=None, return_images: bool = False, return_volume: bool = False):
    """``radius_graph_batch`` on the kernels of csrc/radius.hip (one wavefront per site): the same bonds in the same order
    with the same float32 bond vectors (bit-identical to the torch twin and to the reference's edge lists, tests), every
    crystal on its own cutoff level, ONE host read per batch (total bond count + "did every crystal close its graph").
    CUDA(HIP) device only."""
    from . import _lib
    from ._lib import check, ptr, stream

    lib = _lib.load()
    dev = torch.device(device) if device is not None else torch.as_tensor(fracs[0]).device
    if dev.type != "cuda":
        raise TypeError("radius_graph_batch_hip runs on the GPU; use radius_graph_batch elsewhere")
    B = len(fracs)
    ns = [int(torch.as_tensor(f).shape[0]) for f in fracs]
    N, L = sum(ns), RADIUS_LEVELS
    with _lib.device_guard(torch.empty(0, device=dev)):
        lat64 = torch.stack([torch.as_tensor(x).to(dev, torch.float64) for x in lattices]).contiguous()  # [B,3,3]
        frac64 = torch.cat([torch.as_tensor(f).to(dev, torch.float64) for f in fracs]).contiguous()  # [N,3]
        n_t = torch.tensor(ns, device=dev, dtype=torch.int64)
        gptr = _ptr_from_counts(n_t).to(torch.int32)
        site_graph = torch.repeat_interleave(torch.arange(B, device=dev, dtype=torch.int32), n_t, output_size=N)
        sg = site_graph.long()
        lg = lat64[sg]  # [N,3,3]
        cart32 = (frac64[:, 0:1] * lg[:, 0, :] + frac64[:, 1:2] * lg[:, 1, :] + frac64[:, 2:3] * lg[:, 2, :]).float().contiguous()
        frac32 = frac64.float()
        idx = sg[:, None].expand(-1, 3)
        fmin = torch.full((B, 3), float("inf"), device=dev).scatter_reduce(0, idx, frac32, "amin")
        fmax = torch.full((B, 3), float("-inf"), device=dev).scatter_reduce(0, idx, frac32, "amax")
        spacing = 1.0 / torch.linalg.norm(torch.linalg.inv(lat64), dim=1)  # [B,3] plane spacings
        cuts = float(cutoff) + float(cutoff_extra) * torch.arange(L, device=dev, dtype=torch.float64)  # [L]
        maxr = torch.ceil((cuts[None, :, None] + bond_tol) / spacing[:, None, :] + 1e-9)  # [B,L,3] (see _radius_box)
        nmin = torch.floor(fmin.double())[:, None, :] - maxr
        nmax = torch.ceil(fmax.double())[:, None, :] + maxr
        box = torch.cat([nmin, nmax], 2).to(torch.int32).contiguous()  # [B,L,6]
        cut32 = cuts.float().contiguous()
        lat32 = lat64.float().contiguous()
        level = torch.empty(B, dtype=torch.int32, device=dev)
        count = torch.empty(N, dtype=torch.int64, device=dev)
        st = stream()
        check(lib.alignn_radius_levels(ptr(lat32), ptr(cart32), ptr(gptr), ptr(box), ptr(cut32), float(atol), L, B, ptr(level), st),
              "radius_levels")
        check(lib.alignn_radius_count(ptr(lat32), ptr(cart32), ptr(gptr), ptr(site_graph), ptr(box), ptr(cut32), float(atol), L, N,
                                      ptr(level), ptr(count), st), "radius_count")
        csum = torch.cumsum(count, 0)
        offset = (csum - count).contiguous()
        tail = torch.stack([csum[-1], level.max().to(torch.int64)]).tolist() if N else [0, 0]  # the one host read
        if tail[1] >= L:
            raise RuntimeError(f"radius_graph: a crystal's last site has no neighbour within {cutoff + cutoff_extra * (L - 1)} A")
        E = int(tail[0])
        u = torch.empty(E, dtype=torch.int64, device=dev)
        v = torch.empty(E, dtype=torch.int64, device=dev)
        r = torch.empty(E, 3, dtype=torch.float32, device=dev)
        img = torch.empty(E, 3, dtype=torch.int32, device=dev) if return_images else None
        if E:
            check(lib.alignn_radius_emit(ptr(lat32), ptr(cart32), ptr(gptr), ptr(site_graph), ptr(box), ptr(cut32), float(atol), L, N,
                                         ptr(level), ptr(offset), ptr(u), ptr(v), ptr(r), ptr(img), st), "radius_emit")
        volume = torch.linalg.det(lat64).abs().float() if return_volume else None
    return (u, v, r, ns) + ((img,) if return_images else ()) + ((volume,) if return_volume else ())


KNN_LEVELS = 5  # cutoffs tried per crystal: the given one, then longest lattice vector / doubling (graphs.py:170-188)


# What knn_multigraph_batch_hip derives from the LATTICES alone (cell matrices, per-site crystal index, the ladder of cutoffs
# and image-box half-widths: ~20 small torch operations incl. a batched 3 x 3 inverse).  MD at constant cell (alignn/ff/
# calculators.py rebuilds the graph of the same atoms every step) passes the same lattice tensors again and again: the last
# result is kept, keyed on the tensors' identity and version counters.
# The key covers identity, version counter, storage address, device and dtype of every lattice tensor: an edit through a
# versioned in-place operation (``lat.mul_``, ``lat[0, 0] = ...``) is seen; one that bypasses the version counter
# (``lat.data.copy_``, memory shared with a numpy array that is written to) is NOT - a changing-cell (NPT) run must pass
# fresh tensors, edit through versioned operations, or call ``clear_lattice_cache()`` after such an edit.  Not
# thread-safe (one MD loop per process is the use).
_LATTICE_TABLES = {"key": None, "refs": None, "val": None}


def clear_lattice_cache():
    """Forget the lattice-derived tables kept between calls of ``knn_multigraph_batch_hip`` / ``crystal_batch``."""
    _LATTICE_TABLES.update(key=None, refs=None, val=None)


def _lattice_tables(lattices, ns, dev, cutoff):
    tens = [x for x in lattices if isinstance(x, torch.Tensor)]
    key = None
    if len(tens) == len(lattices):
        key = (tuple((id(x), x._version, x.data_ptr(), x.device, x.dtype) for x in tens), tuple(ns), str(dev), cutoff)
        c = _LATTICE_TABLES
        if c["key"] == key and all(r() is x for r, x in zip(c["refs"], tens)):
            return c["val"]
    B, N = len(ns), sum(ns)
    lat = torch.stack([torch.as_tensor(x).to(dev, torch.float64) for x in lattices]).contiguous()  # [B,3,3]
    n_t = torch.tensor(ns, device=dev, dtype=torch.int64)
    gptr = _ptr_from_counts(n_t).to(torch.int32)
    site_graph = torch.repeat_interleave(torch.arange(B, device=dev, dtype=torch.int32), n_t, output_size=N)
    lg = lat[site_graph.long()].contiguous()  # [N,3,3]
    longest = torch.linalg.norm(lat, dim=2).max(dim=1).values
    spacing = 1.0 / torch.linalg.norm(torch.linalg.inv(lat), dim=1)  # [B,3]
    cuts = [torch.full((B,), float(cutoff), dtype=torch.float64, device=dev)]
    for _ in range(KNN_LEVELS - 1):
        c = cuts[-1]
        cuts.append(torch.where(c < longest, longest, 2.0 * c))
    cut = torch.stack(cuts, 1).contiguous()  # [B,L]
    # the two half-widths _image_box chooses between, per level; the box itself needs the coordinates (alignn_knn_box)
    reach = torch.ceil(cut[:, :, None] / spacing[:, None, :]).to(torch.int32).contiguous()  # [B,L,3]
    maxr = torch.ceil((cut[:, :, None] + BOND_TOL) / spacing[:, None, :]).to(torch.int32).contiguous()
    # (the cell volumes - crystal_batch's GraphBatch.volume - travel WITH the tables: same key, same lifetime)
    val = (lat, gptr, site_graph, lg, cut, reach, maxr, torch.linalg.det(lat).abs().float())
    if key is not None:
        import weakref

        _LATTICE_TABLES.update(key=key, refs=[weakref.ref(x) for x in tens], val=val)
    return val


def knn_multigraph_batch_hip(lattices: Sequence, fracs: Sequence, cutoff: float = 8.0, max_neighbors: int = 12, device=None,
                             return_images: bool = False, return_volume: bool = False):
    """``knn_multigraph_batch`` on the hand-written kernels of csrc/knn.hip (one wavefront per site): the same bond
    list in the same order - bit-identical index arrays, bond vectors equal to rounding - with no padded [B,n,n,I]
    tensors and ONE host read per batch (the total bond count, to size the output).  The image box of every crystal is
    formed on the device from its fractional extent (``alignn_knn_box``); what depends on the lattices alone stays cached
    (``_lattice_tables``).  Raises ``RuntimeError`` when a site lacks ``max_neighbors`` neighbours at the widest of the
    ``KNN_LEVELS`` cutoffs (the reference would go on doubling).  CUDA(HIP) device only."""
    from . import _lib
    from ._lib import check, ptr, stream

    lib = _lib.load()
    dev = torch.device(device) if device is not None else torch.as_tensor(fracs[0]).device
    if dev.type != "cuda":
        raise TypeError("knn_multigraph_batch_hip runs on the GPU; use knn_multigraph_batch elsewhere")
    B = len(fracs)
    ns = [int(torch.as_tensor(f).shape[0]) for f in fracs]
    N = sum(ns)
    with _lib.device_guard(torch.empty(0, device=dev)):
        frac = torch.cat([torch.as_tensor(f).to(dev, torch.float64) for f in fracs]).contiguous()  # [N,3]
        lat, gptr, site_graph, lg, cut, reach, maxr, volume = _lattice_tables(lattices, ns, dev, float(cutoff))
        # the fixed-order float64 product of knn_multigraph / synthetic._all_neighbors (separate multiplies and adds)
        cart = (frac[:, 0:1] * lg[:, 0, :] + frac[:, 1:2] * lg[:, 1, :] + frac[:, 2:3] * lg[:, 2, :]).contiguous()
        level = torch.zeros(B, dtype=torch.int32, device=dev)
        kth = torch.empty(N, dtype=torch.float64, device=dev)
        count = torch.empty(N, dtype=torch.int64, device=dev)
        st = stream()
        L, k = KNN_LEVELS, int(max_neighbors)
        box = torch.empty(B, L, 6, dtype=torch.int32, device=dev)  # image range per crystal and level (_image_box), on the device
        check(lib.alignn_knn_box(ptr(frac), ptr(gptr), ptr(reach), ptr(maxr), L, B, ptr(box), st), "knn_box")
        check(lib.alignn_knn_levels(ptr(lat), ptr(cart), ptr(gptr), ptr(site_graph), ptr(cut), ptr(box), L, k, N, ptr(level),
                                    st), "knn_levels")
        check(lib.alignn_knn_kth(ptr(lat), ptr(cart), ptr(gptr), ptr(site_graph), ptr(cut), ptr(box), L, k, N, ptr(level),
                                 ptr(kth), st), "knn_kth")
        check(lib.alignn_knn_count(ptr(lat), ptr(cart), ptr(gptr), ptr(site_graph), ptr(cut), ptr(box), L, N, ptr(level),
                                   ptr(kth), ptr(count), st), "knn_count")
        csum = torch.cumsum(count, 0)
        offset = (csum - count).contiguous()
        # the one host read: total bonds (sizes the output) and "did every crystal find its k neighbours"
        tail = torch.stack([csum[-1], level.max().to(torch.int64)]).tolist() if N else [0, 0]
        if tail[1] >= L:
            raise RuntimeError(f"a site has fewer than {k} neighbours even at the widest of {L} cutoffs")
        E = 2 * int(tail[0])
        u = torch.empty(E, dtype=torch.int64, device=dev)
        v = torch.empty(E, dtype=torch.int64, device=dev)
        r = torch.empty(E, 3, dtype=torch.float32, device=dev)
        img = torch.empty(E, 3, dtype=torch.int32, device=dev) if return_images else None
        if E:
            check(lib.alignn_knn_emit(ptr(lat), ptr(cart), ptr(gptr), ptr(site_graph), ptr(cut), ptr(box), L, N, ptr(level),
                                      ptr(kth), ptr(offset), ptr(u), ptr(v), ptr(r), ptr(img), st), "knn_emit")
    out = (u, v, r, ns) + ((img,) if return_images else ()) + ((volume,) if return_volume else ())
    return out


def crystal_batch(lattices: Sequence, fracs: Sequence, atom_features: Optional[Sequence] = None, device=None,
                  cutoff: float = 8.0, max_neighbors: int = 12, line_graph: bool = True,
                  neighbor_strategy: str = "k-nearest") -> GraphBatch:
    """Positions -> canonical (g, L(g)) batch, all on the device: one crystal per (lattice, frac) pair; the bond cosines
    are left to the model (``lg_on_fly``) or to ``ops.bond_cosines(batch.r, batch.lg)``.  ``neighbor_strategy``: the
    reference's ``Graph.atom_dgl_multigraph`` switch (alignn/graphs.py:486-505) - "k-nearest" (kNN-``max_neighbors`` within
    ``cutoff``, canonised to an undirected multigraph) or "radius_graph" (every pair within ``cutoff``; what the force-field
    configs use)."""
    dev = torch.device(device) if device is not None else torch.as_tensor(fracs[0]).device
    if neighbor_strategy == "radius_graph":
        volume = None
        if dev.type == "cuda":
            u, v, r, nn, volume = radius_graph_batch_hip(lattices, fracs, cutoff, device=dev, return_volume=True)
        else:
            u, v, r, nn = radius_graph_batch(lattices, fracs, cutoff, device=dev)
    elif neighbor_strategy != "k-nearest":
        raise ValueError(f"neighbor_strategy {neighbor_strategy!r}: 'k-nearest' or 'radius_graph'")
    elif dev.type == "cuda":  # one wave per site (csrc/knn.hip); the torch builder below is its CPU twin and its checker
        u, v, r, nn, volume = knn_multigraph_batch_hip(lattices, fracs, cutoff, max_neighbors, device=dev, return_volume=True)
    else:
        u, v, r, nn = knn_multigraph_batch(lattices, fracs, cutoff, max_neighbors, device=dev)
    off = sum(nn)
    if line_graph:  # (on the GPU: one host read + one C call, graph.csr_and_line_graph)
        g, lg, r_canon = csr_and_line_graph(u, v, off, r)
    else:
        g, lg = build_csr(u, v, off), None
        r_canon = r[g.perm].contiguous()
    gp = torch.zeros(len(nn) + 1, dtype=torch.int32)
    gp[1:] = torch.cumsum(torch.tensor(nn, dtype=torch.int32), 0)  # (on the host: B small integers)
    batch = GraphBatch(g=g, lg=lg, graph_ptr=gp.to(dev), batch_size=len(nn))
    batch.r = r_canon
    if atom_features is not None:
        batch.atom_features = torch.cat([torch.as_tensor(a) for a in atom_features]).to(dev, torch.float32).contiguous()
    if dev.type == "cuda" and volume is not None:  # (derived with - and cached under the same key as - the lattice tables)
        batch.volume = volume
    else:
        lat_t = torch.stack([torch.as_tensor(x).to(dev, torch.float64) for x in lattices])
        batch.volume = torch.linalg.det(lat_t).abs().float()
    return batch
