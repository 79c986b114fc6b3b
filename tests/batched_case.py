"""What the device tests of lfamd_mul_mat_batched and lfamd_mul_mat_batched_q share: device buffers at a chosen misalignment, strided
byte images as ggml hands them over, the sentinel-prefilled result buffer, and one strided call with the two checks that need no
reference — every byte outside the m x n results of each slice unchanged, and bit equality with calls on one slice each."""
import numpy as np

from llamafile_amd import _hip

NAN32 = 0x7fc00000


class Dev:
    """Device buffers through torch; a buffer's base sits `misalign` bytes past a 16-byte boundary."""

    def __init__(self):
        import torch
        self.torch = torch
        self.lib = _hip.lib()

    def put(self, host_u8, misalign):
        t = self.torch.empty(host_u8.size + 48, dtype=self.torch.uint8, device="cuda")
        off = (-t.data_ptr()) % 16 + misalign
        t[off:off + host_u8.size] = self.torch.from_numpy(host_u8).cuda()
        return t, off, host_u8.size

    def ptr(self, h):
        return h[0].data_ptr() + h[1]

    def get(self, h):
        self.torch.cuda.synchronize()
        return h[0][h[1]:h[1] + h[2]].cpu().numpy()


def strided(buf, dtype, shape, strides):
    return np.lib.stride_tricks.as_strided(buf.view(dtype), shape=shape, strides=strides, writeable=True)


def span(shape, strides, elem):
    return sum((e - 1) * s for e, s in zip(shape, strides)) + elem


def b_image(Bv, b_nb, tail_words=0):
    """Bv f32 [ne3][heads][n][k] at the byte strides b_nb = (nb3, nb2, nb1), NaN in every gap."""
    img = np.full(span(Bv.shape, b_nb + (4,), 4) // 4 + tail_words, NAN32, np.uint32)
    strided(img, np.uint32, Bv.shape, b_nb + (4,))[...] = Bv.view(np.uint32)
    return img


def sentinel_c(Csh, c_nb):
    """The result buffer before a call: distinct NaNs, 16 words longer than the results [ne3][heads][n][m] at c_nb need."""
    words = span(Csh, c_nb + (4,), 4) // 4 + 16
    return (np.arange(words, dtype=np.uint64) * 2654435761 % 2 ** 32).astype(np.uint32) | np.uint32(0x7f800001)


def call_on_images(dev, fn, Atype, A_img, B_img, dims, a_nb, b_nb, c_nb, unaligned=False):
    """One call of fn (either entry point) on byte images; dims = (m, k, n, kv heads, a_ne3, heads, ne3), strides as (nb3, nb2, nb1).
    unaligned: A's base 2 bytes, B's and C's 4 bytes past a 16-byte boundary.  Returns the device handles of A and B, the sentinel
    image and the whole result buffer after the call, as uint32."""
    m, k, n, kvh, a_ne3, heads, ne3 = dims
    C_img = sentinel_c((ne3, heads, n, m), c_nb)
    hA = dev.put(A_img.view(np.uint8), 2 if unaligned else 0)
    hB = dev.put(B_img.view(np.uint8), 4 if unaligned else 0)
    hC = dev.put(C_img.view(np.uint8), 4 if unaligned else 0)
    rc = fn(Atype, dev.ptr(hA), m, k, a_nb[2], a_nb[1], a_nb[0], kvh, a_ne3, dev.ptr(hB), n, b_nb[2], b_nb[1], b_nb[0], heads, ne3,
            dev.ptr(hC), c_nb[2], c_nb[1], c_nb[0], 0, None)
    assert rc == 0, _hip.lib().lfamd_last_error()
    return hA, hB, C_img, dev.get(hC).view(np.uint32).copy()


def run_strided_call(dev, fn, Atype, A_img, B_img, dims, a_nb, b_nb, c_nb, unaligned=False):
    """call_on_images, then the two checks; returns the results f32 [ne3][heads][n][m]."""
    m, k, n, kvh, a_ne3, heads, ne3 = dims
    group, Csh = heads // kvh, (ne3, heads, n, m)
    hA, hB, C_img, out = call_on_images(dev, fn, Atype, A_img, B_img, dims, a_nb, b_nb, c_nb, unaligned)
    got = strided(out, np.uint32, Csh, c_nb + (4,)).copy()
    # every byte outside the results is unchanged
    strided(out, np.uint32, Csh, c_nb + (4,))[...] = strided(C_img, np.uint32, Csh, c_nb + (4,))
    assert np.array_equal(out, C_img), "bytes outside the results were written"
    # the same slices by single-slice calls: the same bits
    one = dev.put(np.full(n * m * 4, 0xff, np.uint8), 0)
    for i3 in range(ne3):
        for i2 in range(heads):
            pa = dev.ptr(hA) + (i3 // (ne3 // a_ne3)) * a_nb[0] + (i2 // group) * a_nb[1]
            pb = dev.ptr(hB) + i3 * b_nb[0] + i2 * b_nb[1]
            rc = fn(Atype, pa, m, k, a_nb[2], a_nb[1], a_nb[0], 1, 1, pb, n, b_nb[2], b_nb[1], b_nb[0], 1, 1, dev.ptr(one), m * 4,
                    n * m * 4, n * m * 4, 0, None)
            assert rc == 0, _hip.lib().lfamd_last_error()
            single = dev.get(one).view(np.uint32).reshape(n, m)
            assert np.array_equal(single, got[i3, i2]), ("slice bits depend on the call's other slices", i3, i2)
    return got.view(np.float32)
