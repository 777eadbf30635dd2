"""The list of HIP sources that libp2p_hip.so is built from, and their content hash.

This is the one list: the Makefile takes its ``SRCS`` and ``HDRS`` from here (``--sources`` /
``--headers``) and stamps the hash into the library (``p2p_source_hash()``);
``_hip.check_source_hash`` recomputes it from the tree at run time, so a stale prebuilt binary (the
.so is git-ignored and travels to the GPU box as a file) cannot pass ``smoke()`` or the GPU tests.
Run as a script it prints the hash (the Makefile's ``$(shell ...)``).
"""
import hashlib
import os
import sys

_CSRC = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "csrc")
# one translation unit each, slowest first (make starts them in this order)
SOURCES = ("p2p_generic.hip", "p2p_mutual.hip", "p2p_self40.hip", "p2p_selfmaps.hip", "p2p_selfmulti.hip", "p2p_selfsplit.hip",
           "p2p_selfwide.hip", "p2p_conv.hip", "p2p_linear.hip", "p2p_cross.hip", "p2p_bwd.hip", "p2p_latent.hip", "p2p_blend.hip", "p2p_unet.hip", "p2p_text.hip", "p2p_image.hip", "p2p_viz.hip", "p2p_null.hip", "p2p_dispatch.hip", "p2p_capi.hip")
# what the sources include: the headers, and the two files p2p_generic.hip compiles as one object
HEADERS = ("p2p_device.h", "p2p_kernels.h", "p2p_select.h", "p2p_blend_mask.h", "p2p_mma_tile.h", "p2p_mma_pipe.h",
           "../../include/p2p_hip.h",
           "p2p_self.hip", "p2p_cross_entry.hip")
# every file whose text reaches the compiler or the link line, in a fixed order
FILES = SOURCES + HEADERS + ("Makefile",)


def source_hash() -> str:
    h = hashlib.sha256()
    for name in FILES:
        with open(os.path.join(_CSRC, name), "rb") as f:
            h.update(name.encode())
            h.update(b"\0")
            h.update(f.read())
    return h.hexdigest()[:16]


if __name__ == "__main__":
    if "--sources" in sys.argv:
        print(" ".join(SOURCES))
    elif "--headers" in sys.argv:
        print(" ".join(HEADERS))
    else:
        print(source_hash())
