"""The "batchmcprofile" renderer (BatchMCProfileRenderer, src/renderers/batchmcprofile.cpp:43-141): the
fork's check of its lerp-on-thin-slab extension to the multipole model. The top layer's thickness takes
``thickness_segments + 1`` values between ``thickness_min`` and ``thickness_max``; for each, ``photons``
random walks give the total reflectance and transmittance, and the multipole model gives both without and
with the lerp.

``render(ctx)`` makes three calls on the context's GPU: one batched walk over all thicknesses
(mpss_mc_profile_batch, totals only) and two batched multipole references (mpss_mc_reference_batch, lerp
off, then on, at the reference's desiredLength 1024). It keeps ``results`` (one MCProfileResult-shaped
dict per thickness, mcprofile.h:52-68, in ascending thickness) and writes the reference's seven-column
table when ``filename`` is set.

The reference visits the thicknesses in an interleaved order and sorts afterwards (:52-69); only the sorted
order shows. One deviation: the reference accepts ``thicknessrange`` starting at 0 (and then walks a slab
of no thickness); here a thickness of 0 is refused by the walk's own "thickness > 0" check.
"""
import numpy as np

HEADER = ("Thickness\tMonte-Carlo Reflectance\tMultipole Reflectance\tLerped Reflectance"
          "\tMonte-Carlo Transmittance\tMultipole Transmittance\tLerped Transmittance")
COLUMNS = ("totalMCReflectance", "totalNoLerpReflectance", "totalLerpReflectance",
           "totalMCTransmittance", "totalNoLerpTransmittance", "totalLerpTransmittance")
DESIRED_LENGTH = 1024  # MultipoleReferenceTask::Run, mcprofile.cpp:390


class BatchMCProfileRenderer:
    def __init__(self, layers, mfp_range=16.0, segments=1024, photons=100, thickness_min=0.0, thickness_max=0.0,
                 thickness_segments=256, filename="", seed=89):
        lay = np.asarray(layers, np.float32).reshape(-1, 4)
        if len(lay) < 1:
            raise ValueError("No layers param set for BatchMCProfileRenderer.")
        if not (0.0 <= thickness_min <= thickness_max):
            raise ValueError("Thickness range incorrectly set for BatchMCProfileRenderer.")
        if thickness_segments < 1:
            raise ValueError("BatchMCProfileRenderer: thicknesssegments must be at least 1")
        self.layers = lay
        self.mfp_range = float(np.float32(mfp_range))
        self.segments = int(segments)
        self.photons = int(photons)
        self.thickness_min = float(np.float32(thickness_min))
        self.thickness_max = float(np.float32(thickness_max))
        self.thickness_segments = int(thickness_segments)
        self.filename = filename
        self.seed = seed
        self.results = None

    def thicknesses(self):
        """thicknessMin + (float)ii * (thicknessMax - thicknessMin) / nThicknessSegments in float (:54),
        ii = 0..n ascending."""
        lo, hi = np.float32(self.thickness_min), np.float32(self.thickness_max)
        ii = np.arange(self.thickness_segments + 1).astype(np.float32)
        return (lo + (ii * np.float32(hi - lo)) / np.float32(self.thickness_segments)).astype(np.float32)

    def slabs(self):
        """layers [S, n, 4]: the scene's layers with the top layer's thickness replaced."""
        th = self.thicknesses()
        lay = np.repeat(self.layers[None], len(th), axis=0)
        lay[:, 0, 3] = th
        return lay

    def render(self, ctx, stream=None):
        lay = self.slabs()
        mc = ctx.mc_profile_batch(lay, self.mfp_range, self.segments, self.photons, seed=self.seed, rings=False,
                                  stream=stream)
        ref = [ctx.mc_reference_batch(lay, self.mfp_range, self.segments, lerp, desired_length=DESIRED_LENGTH,
                                      stream=stream) for lerp in (False, True)]
        self.results = [dict(thickness=float(t),
                             totalMCReflectance=float(mc["total_r"][s]), totalMCTransmittance=float(mc["total_t"][s]),
                             totalNoLerpReflectance=float(ref[0]["total_r"][s]),
                             totalNoLerpTransmittance=float(ref[0]["total_t"][s]),
                             totalLerpReflectance=float(ref[1]["total_r"][s]),
                             totalLerpTransmittance=float(ref[1]["total_t"][s]))
                        for s, t in enumerate(lay[:, 0, 3])]
        self.events = mc["events"]
        if self.filename:
            with open(self.filename, "w", newline="\n") as f:
                f.write(tsv(self.results))
        return self.results

    def tsv(self):
        return tsv(self.results)


def tsv(results):
    """The output file of Render (:84-96): numbers as an ostream prints them at its default precision (%g)."""
    out = [HEADER]
    for r in results:
        out.append("\t".join("%g" % r[k] for k in ("thickness",) + COLUMNS))
    return "\n".join(out) + "\n"


def read_tsv(path):
    """Parse a file written by ``tsv`` (or by the reference) back into the list of result dicts."""
    with open(path) as f:
        lines = [l.rstrip("\n") for l in f if l.strip()]
    if lines[0] != HEADER:
        raise ValueError("%s: not a batchmcprofile table" % path)
    res = []
    for l in lines[1:]:
        v = [float(x) for x in l.split("\t")]
        if len(v) != 7:
            raise ValueError("%s: a row of %d fields" % (path, len(v)))
        res.append(dict(zip(("thickness",) + COLUMNS, v)))
    return res


def create_from_params(ps):
    """CreateBatchMCProfileRenderer (:115-141): layers (required), mfprange 16, segments 1024, thicknessrange
    (two floats, 0 <= min <= max), thicknesssegments 256, photons "100" (a string), filename ""."""
    lay = ps.find("layers")
    if lay is None or len(lay) < 4:
        raise ValueError("No layers param set for BatchMCProfileRenderer.")
    layers = [tuple(lay[4 * i:4 * i + 4]) for i in range(len(lay) // 4)]
    tr = ps.find("thicknessrange")
    if tr is None or len(tr) != 2 or tr[0] < 0.0 or tr[1] < tr[0]:
        raise ValueError("Thickness range incorrectly set for BatchMCProfileRenderer.")
    return BatchMCProfileRenderer(layers, float(ps.one("mfprange", 16.0)), int(ps.one("segments", 1024)),
                                  int(str(ps.one("photons", "100"))), float(tr[0]), float(tr[1]),
                                  int(ps.one("thicknesssegments", 256)), str(ps.one("filename", "")))
