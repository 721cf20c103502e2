// prep_resize_body.inc — the statements of the resize kernels (preprocess.hip), included once into each of them: the
// transform of one page behind its ink box, CropWhite(pad) [-> PadToSquare] -> Resize -> ToGray [-> Normalize]. The including
// kernel provides `PrepArgs a` (the page) and `constexpr bool GRAY8` (a.out is uint8 [S, S] and takes the gray byte;
// otherwise fp32 [3, S, S], normalised). ONE text of the pixel arithmetic for prep_resize_kernel (one page) and
// prep_resize_batch_kernel (all pages of a call), so that the two cannot drift — included, not called, for the reason given
// in patch_embed_body.inc: prep_resize_kernel keeps its ISA instruction for instruction.
    const int dx = blockIdx.x * 16 + (threadIdx.x & 15), dy = blockIdx.y * 16 + (threadIdx.x >> 4);
    int top = 0, bottom = a.H, left = 0, right = a.W;
    if (a.bbox[1] >= 0) { top = a.bbox[0]; bottom = a.bbox[1] + 1; left = a.bbox[2]; right = a.bbox[3] + 1; }
    const int hc = bottom - top, wc = right - left;
    if (a.crop_out && blockIdx.x == 0 && blockIdx.y == 0 && threadIdx.x == 0) {
        a.crop_out[0] = top; a.crop_out[1] = a.H - bottom; a.crop_out[2] = left; a.crop_out[3] = a.W - right;
    }
    int Hp = hc + 2 * a.pad, Wp = wc + 2 * a.pad, pad_t = a.pad, pad_l = a.pad;
    if (a.square) {      // PadToSquare after CropWhite (reference data_aug.py:286-301): diff//2 first, the rest after
        const int diff = Hp > Wp ? Hp - Wp : Wp - Hp;
        if (Hp <= Wp) { pad_t += diff / 2; Hp = Wp; } else { pad_l += diff / 2; Wp = Hp; }
    }
    if (dx >= a.S || dy >= a.S) return;
    int y0, y1, wy0, wy1, x0, x1, wx0, wx1;
    linear_tap(dy, Hp, a.S, y0, y1, wy0, wy1);
    linear_tap(dx, Wp, a.S, x0, x1, wx0, wx1);
    auto px = [&](int y, int x, int c) -> int {      // the cropped page with its white border, never materialised
        y -= pad_t; x -= pad_l;
        if (y < 0 || y >= hc || x < 0 || x >= wc) return 255;
        return a.rgb[((size_t)(top + y) * a.W + left + x) * 3 + c];
    };
    int ch[3];
#pragma unroll
    for (int c = 0; c < 3; ++c) {
        const int r0 = px(y0, x0, c) * wx0 + px(y0, x1, c) * wx1;
        const int r1 = px(y1, x0, c) * wx0 + px(y1, x1, c) * wx1;
        const int v = (((wy0 * (r0 >> 4)) >> 16) + ((wy1 * (r1 >> 4)) >> 16) + 2) >> 2;
        ch[c] = min(max(v, 0), 255);
    }
    const int gray = (ch[0] * 4899 + ch[1] * 9617 + ch[2] * 1868 + 8192) >> 14;     // cv2 RGB2GRAY
    if (GRAY8) {
        ((uint8_t*)a.out)[(size_t)dy * a.S + dx] = (uint8_t)(gray & 255);
        return;
    }
    const float g = (float)(gray & 255);
#pragma unroll
    for (int c = 0; c < 3; ++c) a.out[((size_t)c * a.S + dy) * a.S + dx] = (g - a.mean255[c]) * a.inv[c];
