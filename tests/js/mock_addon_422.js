'use strict';
/* tests/js/mock_addon_422.js — TEST INFRASTRUCTURE: tests/js/mock_addon_draw_list.js (left as it is) plus the packed 4:2:2 formats (YUYV = 4,
 * UYVY = 5) in drawFramesYuvDevice, and through it in the mock's drawListDevice: a packed frame — rows of ceil(w / 2) macropixels of 4 bytes,
 * YUYV Y0 U Y1 V, UYVY U Y0 V Y1; pixel (x, y) takes its own Y and the U, V of macropixel x >> 1 of row y — is converted to RGBA by the
 * declared integer rule (restated here: plain int32 arithmetic) and drawn by the mock's RGBA draw, whose counter is put back.  An offset
 * that is no multiple of 4 is refused as csrc/ht_napi.cc refuses it.  Needs withIngest(true), withYuv(true) (and withDrawList(true)). */
const path = require('path');
const mock = require(path.join(__dirname, 'mock_addon_draw_list.js'));
const TABLE = [[16, 298, 409, -100, -208, 516], [16, 298, 459, -55, -136, 541], [0, 256, 359, -88, -183, 454], [0, 256, 403, -48, -120, 475]];
function clamp(v) { return v < 0 ? 0 : v > 255 ? 255 : v; }
function frameBytes(w, h) { return 4 * ((w + 1) >> 1) * h; }
function toRgba(buf, off, w, h, format, matrix) {
  const k = TABLE[matrix], cw = (w + 1) >> 1, out = new Uint8Array(w * h * 4), yo = format === 4 ? 0 : 1, uo = format === 4 ? 1 : 0;
  for (let y = 0; y < h; y++) for (let x = 0; x < w; x++) {
    const m = off + (y * cw + (x >> 1)) * 4, Y = buf[m + yo + 2 * (x & 1)], U = buf[m + uo], V = buf[m + uo + 2];
    const c = k[1] * (Y - k[0]) + 128, d = U - 128, e = V - 128, o = (y * w + x) * 4;
    out[o] = clamp((c + k[2] * e) >> 8); out[o + 1] = clamp((c + k[3] * d + k[4] * e) >> 8); out[o + 2] = clamp((c + k[5] * d) >> 8); out[o + 3] = 255;
  }
  return out;
}
let baseYuv = null;
function packedDraw(c, s, soff, n, w, h, format, matrix, stride, rect, d, doff, dstride, wait) {
  if (format !== 4 && format !== 5) return baseYuv.apply(this, arguments);
  mock.calls.drawFramesYuvDevice = (mock.calls.drawFramesYuvDevice || 0) + 1;
  if (!s || s.kind !== 'dev') throw new TypeError('mock addon: expected a device buffer');
  if (!(matrix >= 0 && matrix <= 3)) throw new Error('mock addon: status -1: matrix');
  if (soff & 3) throw new RangeError('mock addon: srcOffset of a YUYV / UYVY frame must be a multiple of 4');
  const fsz = frameBytes(w, h), ss = stride || fsz;
  if (ss < fsz || (ss & 3)) throw new Error('mock addon: status -1: stride');
  if (soff + (n - 1) * ss + fsz > s.buf.length) throw new RangeError('mock addon: source outside the device buffer');
  const rgba = new Uint8Array(n * w * h * 4);
  for (let f = 0; f < n; f++) rgba.set(toRgba(s.buf, soff + f * ss, w, h, format, matrix), f * w * h * 4);
  const saved = mock.calls.drawFramesDevice;
  try { mock.drawFramesDevice(c, { kind: 'dev', buf: rgba }, 0, n, w, h, 0, 0, rect, d, doff, dstride, false); }
  finally { if (saved === undefined) delete mock.calls.drawFramesDevice; else mock.calls.drawFramesDevice = saved; }
  if (wait) mock.calls.drawFramesYuvDeviceWaited = (mock.calls.drawFramesYuvDeviceWaited || 0) + 1;
}
const withYuv = mock.withYuv;
mock.withYuv = function (on) {
  const m = withYuv.call(mock, on);
  if (on && mock.drawFramesYuvDevice !== packedDraw) { baseYuv = mock.drawFramesYuvDevice; mock.drawFramesYuvDevice = packedDraw; }
  return m;
};
mock.toRgba422 = toRgba;
module.exports = mock;
