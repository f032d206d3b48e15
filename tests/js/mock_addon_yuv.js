'use strict';
/* tests/js/mock_addon_yuv.js — TEST INFRASTRUCTURE: tests/js/mock_addon_ingest.js (left as it is) plus the YUV ingest entry points of
 * csrc/ht_napi.cc — drawFramesYuv, drawFramesYuvDevice — as the declared integer conversion (restated here: plain int32
 * arithmetic, >> 8, clamp) followed by the declared resampler of oracle/canvas_shim.js, so that the host logic of ccv.drawFrames on a
 * YUV video and of ccv.DeviceBatch with opts.sourceFormat runs without a GPU.  tests/test_ingest_yuv_cpu.py compares what comes out
 * with the numpy / oracle expectation of tests/yuv_cases.py.  `withYuv(false)`: an addon that lacks the calls. */
const path = require('path');
const mock = require(path.join(__dirname, 'mock_addon_ingest.js'));
const shim = require(path.join(__dirname, '..', '..', 'oracle', 'canvas_shim.js'));

const TABLE = [[16, 298, 409, -100, -208, 516], [16, 298, 459, -55, -136, 541], [0, 256, 359, -88, -183, 454], [0, 256, 403, -48, -120, 475]];
function count(name) { mock.calls[name] = (mock.calls[name] || 0) + 1; }
function live(c) { if (!c || c.kind !== 'ctx' || c.destroyed) throw new TypeError('mock addon: expected a live context'); return c; }
function dev(d) { if (!d || d.kind !== 'dev' || !d.buf) throw new TypeError('mock addon: expected a live device buffer'); return d; }
function clamp(v) { return v < 0 ? 0 : v > 255 ? 255 : v; }
function frameBytes(w, h) { return w * h + 2 * ((w + 1) >> 1) * ((h + 1) >> 1); }

/* one packed frame at S[off ..] -> Uint8Array RGBA of w x h */
function toRgba(S, off, w, h, format, matrix) {
  if (format !== 0 && format !== 1) throw new Error('mock addon: status -1: format');
  const k = TABLE[matrix];
  if (!k) throw new Error('mock addon: status -1: matrix');
  const cw = (w + 1) >> 1, ch = (h + 1) >> 1, cbase = off + w * h, out = new Uint8Array(w * h * 4);
  if (format === 0 && (cbase & 1)) throw new Error('mock addon: status -1: the NV12 chroma plane must start at an even address');
  for (let y = 0; y < h; y++) {
    for (let x = 0; x < w; x++) {
      const ci = (y >> 1) * cw + (x >> 1);
      const U = format === 0 ? S[cbase + 2 * ci] : S[cbase + ci], V = format === 0 ? S[cbase + 2 * ci + 1] : S[cbase + cw * ch + ci];
      const C = (S[off + y * w + x] - k[0]) * k[1], D = U - 128, E = V - 128, o = 4 * (y * w + x);
      out[o] = clamp((C + k[2] * E + 128) >> 8);
      out[o + 1] = clamp((C + k[3] * D + k[4] * E + 128) >> 8);
      out[o + 2] = clamp((C + k[5] * D + 128) >> 8);
      out[o + 3] = 255;
    }
  }
  return out;
}
function rectOf(rect, sw, sh) {
  if (rect === null || rect === undefined) return [0, 0, sw, sh];
  if (!(rect instanceof Int32Array) || rect.length < 4) throw new TypeError('mock addon: rect is an Int32Array [x, y, width, height] or null');
  if (rect[0] < 0 || rect[1] < 0 || rect[2] <= 0 || rect[3] <= 0 || rect[0] + rect[2] > sw || rect[1] + rect[3] > sh) throw new Error('mock addon: status -1: rect outside the source frame');
  return [rect[0], rect[1], rect[2], rect[3]];
}
function drawInto(c, S, soff, sstride, n, w, h, format, matrix, rect, D, doff, dstride) {
  if (!(c.w > 0 && c.h > 0)) throw new Error('mock addon: status -6: no geometry');
  if (format === 0 && n > 1 && (sstride & 1)) throw new Error('mock addon: status -1: odd NV12 frame stride');
  const r = rectOf(rect, w, h), fb = c.w * c.h * 4;
  for (let f = 0; f < n; f++) {
    const src = toRgba(S, soff + f * sstride, w, h, format, matrix), dst = new Uint8ClampedArray(fb);
    shim.resample(src, w, h, r[0], r[1], r[2], r[3], dst, c.w, c.h, 0, 0, c.w, c.h);
    D.set(dst, doff + f * dstride);
  }
}

const yuv = {
  drawFramesYuv: function (c, data, n, w, h, format, matrix, rect) {
    count('drawFramesYuv'); live(c);
    if (n > c.maxBatch) throw new Error('mock addon: status -1: more frames than the batch capacity');
    if (data.length < n * frameBytes(w, h)) throw new RangeError('mock addon: planes too short');
    const fb = c.w * c.h * 4, own = new Uint8Array(n * fb);
    /* (the library stages an odd NV12 frame one byte into its buffer; the mock converts from a copy at offset 0 / 1 likewise) */
    const lead = format === 0 ? (frameBytes(w, h) & 1) : 0, step = frameBytes(w, h) + lead, staged = new Uint8Array(lead + n * step);
    for (let f = 0; f < n; f++) staged.set(data.subarray(f * frameBytes(w, h), (f + 1) * frameBytes(w, h)), lead + f * step);
    drawInto(c, staged, lead, step, n, w, h, format, matrix, rect, own, 0, fb);
    c.frames = own; c.n = n; c.stride = fb;
  },
  drawFramesYuvDevice: function (c, s, soff, n, w, h, format, matrix, stride, rect, d, doff, dstride, wait) {
    count('drawFramesYuvDevice'); live(c); dev(s);
    const fb = c.w * c.h * 4, fsz = frameBytes(w, h), ss = stride || fsz;
    if (ss < fsz) throw new Error('mock addon: status -1: stride smaller than a frame');
    if (soff + (n - 1) * ss + fsz > s.buf.length) throw new RangeError('mock addon: source outside the device buffer');
    if (d === null || d === undefined) {
      if (n > c.maxBatch) throw new Error('mock addon: status -1: more frames than the batch capacity');
      const own = new Uint8Array(n * fb);
      drawInto(c, s.buf, soff, ss, n, w, h, format, matrix, rect, own, 0, fb);
      c.frames = own; c.n = n; c.stride = fb;
      return;
    }
    dev(d);
    const ds = dstride || fb;
    if (doff + (n - 1) * ds + fb > d.buf.length) throw new RangeError('mock addon: destination outside the device buffer');
    drawInto(c, s.buf, soff, ss, n, w, h, format, matrix, rect, d.buf, doff, ds);
    if (wait) count('drawFramesYuvDeviceWaited');
  }
};

mock.withYuv = function (on) {
  Object.keys(yuv).forEach(function (k) { if (on) mock[k] = yuv[k]; else delete mock[k]; });
  return mock;
};
module.exports = mock;
