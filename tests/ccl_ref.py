"""Connected components as include/pdeip.h defines them, restated in plain NumPy / Python: a column-major flood fill that shares
nothing with the kernels.  The checker of tests/test_gpu_ccl.py; itself checked against scipy.ndimage.label in test_ccl_ref.py."""
import numpy as np

OFFSETS = {4: ((-1, 0), (1, 0), (0, -1), (0, 1)),
           8: ((-1, -1), (-1, 0), (-1, 1), (0, -1), (0, 1), (1, -1), (1, 0), (1, 1))}


def foreground(A):
    """A > 0 as the contract reads it: NaN, both zeros and negatives are background."""
    with np.errstate(invalid="ignore"):
        return np.asarray(A) > 0


def label(A, conn=8):
    """(L int32 [rows, cols], num, areas int32 [num]): components numbered in the order of their first pixel in column-major order."""
    fg = foreground(A)
    rows, cols = fg.shape
    L = np.zeros((rows, cols), np.int32)
    areas = []
    offs = OFFSETS[conn]
    for j in range(cols):
        for i in np.flatnonzero(fg[:, j] & (L[:, j] == 0)):
            if L[i, j]:
                continue
            lab = len(areas) + 1
            L[i, j] = lab
            stack = [(int(i), j)]
            n = 0
            while stack:
                a, b = stack.pop()
                n += 1
                for da, db in offs:
                    c, d = a + da, b + db
                    if 0 <= c < rows and 0 <= d < cols and fg[c, d] and not L[c, d]:
                        L[c, d] = lab
                        stack.append((c, d))
            areas.append(n)
    return L, len(areas), np.asarray(areas, np.int32)


def largest_component(A, conn=8, hi=1.0, lo=0.0):
    """(plane float32, num, area): hi on the component of the largest area (the lowest label on a tie), lo elsewhere."""
    L, num, areas = label(A, conn)
    out = np.full(L.shape, lo, np.float32)
    if num == 0:
        return out, 0, 0
    best = int(np.argmax(areas))  # the first maximum
    out[L == best + 1] = hi
    return out, num, int(areas[best])
