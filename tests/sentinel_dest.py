"""A sentinel-filled destination for the conv kernels' GPU tests: whatever a launch writes outside the region it was given
shows up as a float that no longer holds the sentinel.  Imported by the tests of the Winograd epilogue and of the generic
kernel's instantiations."""
import torch

SENT = -7.25            # exact in fp32 and in half; no conv in these tests produces it


class Dest:
    """A flat sentinel buffer and a [B, H, W, cout] conv output inside it: `head` elements, then per image H * W pixels of
    `cstride` elements of which [coff, coff + cout) are the conv's and `bgap` spare elements, then `tail` elements.
    `view` is the `out_view` of ops.conv2d (a per-image batch stride); `out` / `coff` are its `out` / `out_coff` (bgap = 0:
    the [B, H, W, cstride] tensor inside the buffer, no batch stride)."""

    def __init__(self, shape, cout, cstride, coff=0, head=0, tail=8, bgap=0, dtype=torch.float32):
        self.B, self.H, self.W = shape
        self.cout, self.cstride, self.coff, self.head, self.bgap = cout, cstride, coff, head, bgap
        assert coff + cout <= cstride
        self.npix = self.B * self.H * self.W
        self.bstride = self.H * self.W * cstride + bgap
        self.buf = torch.full((head + self.B * self.bstride + tail,), SENT, device="cuda", dtype=dtype)
        self.view = (self.buf, head + coff, cstride, self.bstride)

    @property
    def out(self):
        assert self.bgap == 0
        return self.buf[self.head:self.head + self.npix * self.cstride].view(self.B, self.H, self.W, self.cstride)

    def read(self):
        """-> the conv's values [B, H, W, cout]; asserts that every other element still holds the sentinel."""
        torch.cuda.synchronize()
        flat = self.buf.cpu().numpy()
        end = self.head + self.B * self.bstride
        assert (flat[:self.head] == SENT).all() and (flat[end:] == SENT).all()
        imgs = flat[self.head:end].reshape(self.B, self.bstride)
        assert (imgs[:, self.bstride - self.bgap:] == SENT).all()
        body = imgs[:, :self.bstride - self.bgap].reshape(self.npix, self.cstride)
        assert (body[:, :self.coff] == SENT).all() and (body[:, self.coff + self.cout:] == SENT).all()
        return body[:, self.coff:self.coff + self.cout].reshape(self.B, self.H, self.W, self.cout).copy()
