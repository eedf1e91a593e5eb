"""Plain fp64 references of the operators' neighbour kernels (mhla_amd/csrc/epilogue.hpp, lepe.hpp), written from the
definition of each operation.  Every reference evaluates on the given tensors after .double(): give it the (rounded) values
the kernel sees, as fp64 leaves that require grad, and autograd supplies the gradients.  test_neighbour_refs_cpu.py pins each
of them to the oracle; test_gpu_neighbours.py holds the HIP kernels to them."""
import torch
import torch.nn.functional as F


def rmsnorm_gate_ref(x, g, w, eps):
    """y = x / sqrt(mean(x^2, -1) + eps) [* w] [* g * sigmoid(g)] over the last dim; g and w may be None."""
    xd = x.double()
    y = xd / torch.sqrt(xd.square().mean(-1, keepdim=True) + eps)
    if w is not None:
        y = y * w.double()
    if g is not None:
        gd = g.double()
        y = y * gd * torch.sigmoid(gd)
    return y


def _feature_map(x, fmap):
    if fmap in (None, "identity"):
        return x
    if fmap == "relu":
        return torch.relu(x)
    if fmap == "elu":
        return F.elu(x) + 1.0
    raise ValueError(fmap)


def featmap_rotary_ref(x, cos, sin, fmap, off):
    """Feature map (None / "relu" / "elu" = elu + 1), then the NeoX rotary: the halves (x[i], x[i + K/2]) of a head rotate by the
    angle of token off + t.  x [B, T, H, K]; cos, sin [>= off + T, K/2] are used as stored (the activation dtype's values)."""
    T = x.shape[1]
    c = cos.double()[off:off + T][None, :, None, :]
    s = sin.double()[off:off + T][None, :, None, :]
    a, b = _feature_map(x.double(), fmap).chunk(2, dim=-1)
    return torch.cat((a * c - b * s, b * c + a * s), dim=-1)


def qk_prologue_ref(x, w, norm_eps, eps, rope=None, head_dim=None):
    """y = relu(x / sqrt(mean(x^2, -1) + norm_eps) * w) + eps over the last dim C (w None: relu(x) + eps, no norm) and, with
    rope=(cos, sin) [ntok, head_dim / 2], y_rope: the consecutive channel pairs (2i, 2i + 1) of every head rotated by the angles
    of token = row % ntok, rows = all leading dims flattened.  Returns (y, y_rope); y_rope is None without rope."""
    xd = x.double()
    if w is not None:
        xd = xd / torch.sqrt(xd.square().mean(-1, keepdim=True) + norm_eps) * w.double()
    y = torch.relu(xd) + eps
    if rope is None:
        return y, None
    cos, sin = (t.double() for t in rope)
    C = x.shape[-1]
    ntok = cos.shape[0]
    y2 = y.reshape(-1, C // head_dim, head_dim // 2, 2)
    tok = torch.arange(y2.shape[0]) % ntok
    c, s = cos[tok][:, None, :], sin[tok][:, None, :]
    y0, y1 = y2[..., 0], y2[..., 1]
    yr = torch.stack((y0 * c - y1 * s, y0 * s + y1 * c), dim=-1)
    return y, yr.reshape(y.shape)


def rms_rstd_ref(x, norm_eps):
    """1 / sqrt(mean(x^2, -1) + norm_eps), one number per row."""
    return 1.0 / torch.sqrt(x.double().square().mean(-1) + norm_eps)


def blocks_to_image(t, pl, bl):
    """[B, N, C] in block-major token order (token (py * pl + px) * bl^2 + by * bl + bx is pixel (py * bl + by, px * bl + bx))
    -> [B, C, side, side], side = pl * bl."""
    B, N, C = t.shape
    return t.reshape(B, pl, pl, bl, bl, C).permute(0, 5, 1, 3, 2, 4).reshape(B, C, pl * bl, pl * bl)


def image_to_blocks(t, pl, bl):
    """The inverse of blocks_to_image: [B, C, side, side] -> [B, N, C]."""
    B, C = t.shape[:2]
    return t.reshape(B, C, pl, bl, pl, bl).permute(0, 2, 4, 3, 5, 1).reshape(B, (pl * bl) ** 2, C)


def raster_to_video(t, grid):
    """[B, N, C] in raster token order n = (f * H + h) * W + w -> [B, C, F, H, W]."""
    B, N, C = t.shape
    return t.reshape(B, *grid, C).permute(0, 4, 1, 2, 3)


def video_to_raster(t):
    B, C = t.shape[:2]
    return t.permute(0, 2, 3, 4, 1).reshape(B, -1, C)


def lepe2d_ref(v, weight, bias, add, pl, bl):
    """conv2d(v as image, weight [C, 1, K, K], bias, zero padding K // 2, groups = C) [+ add] on block-major tokens [B, N, C]."""
    C, K = weight.shape[0], weight.shape[-1]
    y = F.conv2d(blocks_to_image(v.double(), pl, bl), weight.double(), None if bias is None else bias.double(), padding=K // 2, groups=C)
    y = image_to_blocks(y, pl, bl)
    return y if add is None else y + add.double()


def lepe3d_ref(v, weight, bias, add, grid):
    """conv3d(v as video, weight [C, 1, 3, 3, 3], bias, zero padding 1, groups = C) [+ add] on raster tokens [B, N, C]."""
    C = weight.shape[0]
    y = F.conv3d(raster_to_video(v.double(), grid), weight.double(), None if bias is None else bias.double(), padding=1, groups=C)
    y = video_to_raster(y)
    return y if add is None else y + add.double()
