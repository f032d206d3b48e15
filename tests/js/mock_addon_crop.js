'use strict';
/* tests/js/mock_addon_crop.js — TEST INFRASTRUCTURE: tests/js/mock_addon_draw_list.js and tests/js/mock_addon_pairs.js (both left as they are;
 * they extend the same mock object) plus the crop entry points of csrc/ht_napi.cc — cropPairsDevice, cropSourcesDevice, cropResult — so that
 * the host logic of ccv.DeviceBatch's cropPairs / cropFeeds / cropResult runs without a GPU.  The track object is read from the oracle's
 * tracker state; the rule is restated here in BigInt (floor and ceiling divisions written out); the patch is the mock's single-source draw
 * (the declared conversion and resampler) onto a canvas of the patch size — today's host route.  Needs withIngest, withYuv, withDrawList.
 * `withCrop(false)`: an addon that lacks the calls. */
const path = require('path');
const mock = require(path.join(__dirname, 'mock_addon_draw_list.js'));
require(path.join(__dirname, 'mock_addon_pairs.js'));
const DRAW_RGBA = 16, OBJ_OFFSET = 4096 * 4 + 4 * 4; /* ho_cs_state: model, search window, then x, y, width, height, angle */

function live(c) { if (!c || c.kind !== 'ctx' || c.destroyed) throw new TypeError('mock addon: expected a live context'); return c; }
function floorI32(v) { if (v !== v) return 0; if (v >= 2147483647) return 2147483647; if (v <= -2147483648) return -2147483648; return Math.floor(v); }
function fdiv(a, b) { const q = a / b; return (a % b !== 0n && a < 0n) ? q - 1n : q; }
function cdiv(a, b) { const q = a / b; return (a % b !== 0n && a > 0n) ? q + 1n : q; }
function rule(obj, W, H, SW, SH, m, margin, flags) {
  const cx = floorI32(obj[0]), cy = floorI32(obj[1]), w = floorI32(obj[2]), h = floorI32(obj[3]);
  if (w <= 0 || h <= 0 || w > 65536 || h > 65536 || Math.abs(cx) > 1048576 || Math.abs(cy) > 1048576) return null;
  const B = BigInt, q = B(margin);
  const L = 512n * B(cx) - B(w) * q, R = 512n * B(cx) + B(w) * q, T = 512n * B(cy) - B(h) * q, Bo = 512n * B(cy) + B(h) * q;
  let l = B(m[0]) + fdiv(L * B(m[2]), 512n * B(W)), r = B(m[0]) + cdiv(R * B(m[2]), 512n * B(W));
  let t = B(m[1]) + fdiv(T * B(m[3]), 512n * B(H)), b = B(m[1]) + cdiv(Bo * B(m[3]), 512n * B(H));
  if (flags & 1) {
    const dw = r - l, dh = b - t;
    if (dw < dh) { l -= fdiv(dh - dw, 2n); r = l + dh; } else if (dh < dw) { t -= fdiv(dw - dh, 2n); b = t + dw; }
  }
  if (l < 0n) l = 0n; if (t < 0n) t = 0n; if (r > B(SW)) r = B(SW); if (b > B(SH)) b = B(SH);
  if (r <= l || b <= t) return null;
  return [Number(l), Number(t), Number(r - l), Number(b - t)];
}
function objOf(c, s) {
  if (s < 0 || s >= c.cs.length) throw new Error('mock addon: status -1: stream ' + s + ' is not reserved');
  const st = c.cs[s];
  if (!st) return [0, 0, 0, 0];
  const v = new DataView(st.buffer, st.byteOffset);
  return [0, 1, 2, 3].map(function (k) { return v.getFloat64(OBJ_OFFSET + 8 * k, true); });
}
function params(prm) {
  if (!(prm instanceof Int32Array) || prm.length !== 4) throw new TypeError('mock addon: params is an Int32Array [width, height, marginQ8, flags]');
  if (prm[0] < 1 || prm[0] > 1024 || prm[1] < 1 || prm[1] > 1024) throw new RangeError('mock addon: width and height are 1..1024');
  if (prm[2] < 64 || prm[2] > 1024 || (prm[3] & ~1)) throw new Error('mock addon: status -1: margin_q8 must be 64..1024, flags 0 or 1');
  return { w: prm[0], h: prm[1], margin: prm[2], flags: prm[3] };
}
/* entries: [{stream, dev, offset, SW, SH, format, matrix, mapping}] */
function run(c, entries, p, out, ostride, ooff) {
  if (!out || out.kind !== 'dev' || !out.buf) throw new TypeError('mock addon: expected a live device buffer');
  if (!c.cs || !c.cs.length) throw new Error('mock addon: status -6: call camshiftReserve first');
  const pb = p.w * p.h * 4, stride = ostride || pb, off = ooff || 0, n = entries.length;
  if (off + (n - 1) * stride + pb > out.buf.length) throw new RangeError('mock addon: output outside the device buffer');
  const recs = entries.map(function (e, i) {
    const rect = rule(objOf(c, e.stream), c.w, c.h, e.SW, e.SH, e.mapping, p.margin, p.flags);
    return { i: i, e: e, rect: rect };
  });
  const fake = { kind: 'ctx', w: p.w, h: p.h, maxBatch: 1 }, saved = Object.assign({}, mock.calls);
  try {
    recs.forEach(function (r) {
      const at = off + r.i * stride;
      if (!r.rect) { out.buf.fill(0, at, at + pb); return; }
      const rect = Int32Array.from(r.rect);
      if (r.e.format === DRAW_RGBA) mock.drawFramesDevice(fake, r.e.dev, r.e.offset, 1, r.e.SW, r.e.SH, 0, 0, rect, out, at, 0, false);
      else mock.drawFramesYuvDevice(fake, r.e.dev, r.e.offset, 1, r.e.SW, r.e.SH, r.e.format, r.e.matrix || 0, 0, rect, out, at, 0, false);
    });
  } finally {
    Object.keys(mock.calls).forEach(function (k) { if (k in saved) mock.calls[k] = saved[k]; else delete mock.calls[k]; });
  }
  c.crop = { n: n, records: new Int32Array(6 * n), ratios: new Float64Array(2 * n) };
  recs.forEach(function (r) {
    c.crop.records.set([r.rect ? 1 : 0, r.e.stream].concat(r.rect || [0, 0, 0, 0]), 6 * r.i);
    if (r.rect) { c.crop.ratios[2 * r.i] = r.rect[2] / p.w; c.crop.ratios[2 * r.i + 1] = r.rect[3] / p.h; }
  });
}

const crop = {
  CROP_EMPTY: 0, CROP_FACE: 1, CROP_SQUARE: 1,
  cropPairsDevice: function (c, pairs, prm, out, ostride, ooff, wait) {
    mock.calls.cropPairsDevice = (mock.calls.cropPairsDevice || 0) + 1; live(c);
    if (!(pairs instanceof Int32Array) || pairs.length < 2 || (pairs.length & 1)) throw new TypeError('mock addon: cropPairsDevice(ctx, Int32Array pairs[2n], ...)');
    const p = params(prm);
    if (!c.frames || c.n < 1) throw new Error('mock addon: status -6: bind frames first');
    const entries = [];
    for (let i = 0; i < pairs.length >> 1; i++) {
      const f = pairs[2 * i + 1];
      if (f < 0 || f >= c.n) throw new Error('mock addon: status -1: entry ' + i + ': frame ' + f + ' is not bound');
      entries.push({ stream: pairs[2 * i], dev: { kind: 'dev', buf: c.frames }, offset: f * c.stride, SW: c.w, SH: c.h, format: DRAW_RGBA, matrix: 0, mapping: [0, 0, c.w, c.h] });
    }
    run(c, entries, p, out, ostride, ooff);
  },
  cropSourcesDevice: function (c, streams, list, prm, out, ostride, ooff, wait) {
    mock.calls.cropSourcesDevice = (mock.calls.cropSourcesDevice || 0) + 1; live(c);
    if (!(streams instanceof Int32Array) || !Array.isArray(list) || list.length < 1 || streams.length !== list.length) throw new TypeError('mock addon: cropSourcesDevice(ctx, Int32Array streams[n], entries[n], ...)');
    const p = params(prm);
    const entries = list.map(function (e, i) {
      const whole = !e.rect || (e.rect[2] === 0 && e.rect[3] === 0);
      const m = whole ? [0, 0, e.width, e.height] : Array.from(e.rect);
      if (m[0] < 0 || m[1] < 0 || m[2] <= 0 || m[3] <= 0 || m[0] + m[2] > e.width || m[1] + m[3] > e.height) throw new Error('mock addon: status -1: entry ' + i + ': source rect must lie wholly inside the source frame');
      return { stream: streams[i], dev: e.dev, offset: e.offset || 0, SW: e.width, SH: e.height, format: e.format, matrix: e.matrix, mapping: m };
    });
    run(c, entries, p, out, ostride, ooff);
  },
  cropResult: function (c, n) {
    mock.calls.cropResult = (mock.calls.cropResult || 0) + 1; live(c);
    if (!c.crop) throw new Error('mock addon: status -6: no crop call to report on');
    if (n !== c.crop.n) throw new Error('mock addon: status -6: n differs from the last crop call');
    return { records: Int32Array.from(c.crop.records), ratios: Float64Array.from(c.crop.ratios) };
  }
};
if (typeof mock.deviceDownload !== 'function')
  mock.deviceDownload = function (c, d, off, dst) { live(c); if (!d || !d.buf || off + dst.length > d.buf.length) throw new RangeError('mock addon: outside the device buffer'); dst.set(d.buf.subarray(off, off + dst.length)); };

mock.withCrop = function (on) {
  Object.keys(crop).forEach(function (k) { if (on) mock[k] = crop[k]; else delete mock[k]; });
  return mock;
};
module.exports = mock;
