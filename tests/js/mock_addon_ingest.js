'use strict';
/* tests/js/mock_addon_ingest.js — TEST INFRASTRUCTURE: tests/js/mock_addon.js (left as it is) plus the ingest entry points of
 * csrc/ht_napi.cc — drawFrames, drawFramesDevice, deviceDownload — on the declared resampler of oracle/canvas_shim.js, so that the host
 * logic of ccv.drawFrames and of ccv.DeviceBatch's uploadSource / draw / drawBound runs without a GPU.  `withIngest(false)` is the plain
 * mock: an addon that lacks the calls, for the facade's fallback. */
const path = require('path');
const mock = require(path.join(__dirname, 'mock_addon.js'));
const shim = require(path.join(__dirname, '..', '..', 'oracle', 'canvas_shim.js'));

function count(name) { mock.calls[name] = (mock.calls[name] || 0) + 1; }
function live(c) { if (!c || c.kind !== 'ctx' || c.destroyed) throw new TypeError('mock addon: expected a live context'); return c; }
function dev(d) { if (!d || d.kind !== 'dev' || !d.buf) throw new TypeError('mock addon: expected a live device buffer'); return d; }
function rectOf(rect, sw, sh) {
  if (rect === null || rect === undefined) return [0, 0, sw, sh];
  if (!(rect instanceof Int32Array) || rect.length < 4) throw new TypeError('mock addon: rect is an Int32Array [x, y, width, height] or null');
  if (rect[0] < 0 || rect[1] < 0 || rect[2] <= 0 || rect[3] <= 0 || rect[0] + rect[2] > sw || rect[1] + rect[3] > sh) throw new Error('mock addon: status -1: rect outside the source frame');
  return [rect[0], rect[1], rect[2], rect[3]];
}
/* n frames of sw x sh (rows packed, frames sstride apart) -> n frames of the context's geometry, frames dstride apart */
function drawInto(c, S, soff, sstride, n, sw, sh, rect, D, doff, dstride) {
  if (!(c.w > 0 && c.h > 0)) throw new Error('mock addon: status -6: no geometry');
  const r = rectOf(rect, sw, sh), fb = c.w * c.h * 4;
  for (let f = 0; f < n; f++) {
    const src = S.subarray(soff + f * sstride, soff + f * sstride + sw * sh * 4), dst = new Uint8ClampedArray(fb);
    shim.resample(src, sw, sh, r[0], r[1], r[2], r[3], dst, c.w, c.h, 0, 0, c.w, c.h);
    D.set(dst, doff + f * dstride);
  }
}

const ingest = {
  deviceDownload: function (c, d, off, dst) {
    count('deviceDownload'); live(c); dev(d);
    if (off + dst.length > d.buf.length) throw new RangeError('mock addon: outside the device buffer');
    dst.set(d.buf.subarray(off, off + dst.length));
  },
  drawFrames: function (c, data, n, sw, sh, rect) {
    count('drawFrames'); live(c);
    if (n > c.maxBatch) throw new Error('mock addon: status -1: more frames than the batch capacity');
    const fb = c.w * c.h * 4, own = new Uint8Array(n * fb);
    drawInto(c, data, 0, sw * sh * 4, n, sw, sh, rect, own, 0, fb);
    c.frames = own; c.n = n; c.stride = fb;
  },
  drawFramesDevice: function (c, s, soff, n, sw, sh, pitch, stride, rect, d, doff, dstride, wait) {
    count('drawFramesDevice'); live(c); dev(s);
    if (pitch !== 0 && pitch !== sw * 4) throw new Error('mock addon: only packed rows');
    const fb = c.w * c.h * 4, ss = stride || sw * sh * 4;
    if (soff + (n - 1) * ss + sw * sh * 4 > s.buf.length) throw new RangeError('mock addon: source outside the device buffer');
    if (d === null || d === undefined) {
      if (n > c.maxBatch) throw new Error('mock addon: status -1: more frames than the batch capacity');
      const own = new Uint8Array(n * fb);
      drawInto(c, s.buf, soff, ss, n, sw, sh, rect, own, 0, fb);
      c.frames = own; c.n = n; c.stride = fb;
      return;
    }
    dev(d);
    const ds = dstride || fb;
    if (doff + (n - 1) * ds + fb > d.buf.length) throw new RangeError('mock addon: destination outside the device buffer');
    drawInto(c, s.buf, soff, ss, n, sw, sh, rect, d.buf, doff, ds);
    if (wait) count('drawFramesDeviceWaited');
  }
};

mock.withIngest = function (on) {
  Object.keys(ingest).forEach(function (k) { if (on) mock[k] = ingest[k]; else delete mock[k]; });
  return mock;
};
module.exports = mock;
