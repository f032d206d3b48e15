'use strict';
/* tests/js/mock_addon_align.js — TEST INFRASTRUCTURE: tests/js/mock_addon_crop.js (left as it is; it extends the same mock object) plus the
 * aligned-crop entry points of csrc/ht_napi.cc — alignPairsDevice, alignSourcesDevice, alignResult — so that the host logic of
 * ccv.DeviceBatch's alignPairs / alignFeeds / alignResult runs without a GPU.  The track object (angle included) is read from the oracle's
 * tracker state; the rule is restated here in BigInt (floor divisions and arithmetic shifts written out), the quarter-wave table comes from
 * Math.sin and is checked against the CRC-32 of its description; the patch is sampled from the source's declared RGBA view.  Needs
 * withIngest, withYuv, withDrawList, withCrop.  `withAlign(false)`: an addon that lacks the calls. */
const path = require('path');
const mock = require(path.join(__dirname, 'mock_addon_crop.js'));
const DRAW_RGBA = 16, OBJ_OFFSET = 4096 * 4 + 4 * 4; /* ho_cs_state: model, search window, then x, y, width, height, angle */
const K = 1303.7972938088067; /* the binary64 nearest to 8192 / (2 pi) */
const YUV = [[16, 298, 409, -100, -208, 516], [16, 298, 459, -55, -136, 541], [0, 256, 359, -88, -183, 454], [0, 256, 403, -48, -120, 475]];

const T = new Int32Array(1025);
for (let k = 0; k <= 1024; k++) T[k] = Math.round(Math.sin(k * Math.PI / 2048) * 1073741824);
(function () {
  let c = -1;
  const b = new Uint8Array(T.buffer);
  for (let i = 0; i < b.length; i++) { c ^= b[i]; for (let k = 0; k < 8; k++) c = (c & 1) ? (0xEDB88320 ^ (c >>> 1)) : (c >>> 1); }
  if (((c ^ -1) >>> 0) !== 3814055822) throw new Error('mock addon: the sine table of this JavaScript engine is not the described one');
})();
function sinQ30(a) { const q = a >> 10, r = a & 1023; return BigInt([T[r], T[1024 - r], -T[r], -T[1024 - r]][q]); }

function live(c) { if (!c || c.kind !== 'ctx' || c.destroyed) throw new TypeError('mock addon: expected a live context'); return c; }
function floorI32(v) { if (v !== v) return 0; if (v >= 2147483647) return 2147483647; if (v <= -2147483648) return -2147483648; return Math.floor(v); }
function fdiv(a, b) { const q = a / b; return (a % b !== 0n && a < 0n) ? q - 1n : q; }
/* -> null (empty) or {a12, t: [Cx, Cy, UxS, UyS, VxS, VyS] as BigInt} */
function plan(obj, W, H, m, margin, flags) {
  const cx = floorI32(obj[0]), cy = floorI32(obj[1]), w = floorI32(obj[2]), h = floorI32(obj[3]), angle = obj[4];
  if (w <= 0 || h <= 0 || w > 65536 || h > 65536 || Math.abs(cx) > 1048576 || Math.abs(cy) > 1048576) return null;
  if (!(angle >= -1024 && angle <= 1024)) return null;
  const a12 = ((floorI32(angle * K) + 1) >> 1) & 4095, B = BigInt;
  const S = sinQ30(a12), C = sinQ30((a12 + 1024) & 4095);
  let bw = B(w) * B(margin), bh = B(h) * B(margin);
  if (flags & 1) { if (bw < bh) bw = bh; else bh = bw; }
  const Ux = (bw * S) >> 22n, Uy = (-bw * C) >> 22n, Vx = (bh * C) >> 22n, Vy = (bh * S) >> 22n; /* BigInt >> is arithmetic: floor */
  return { a12: a12, t: [B(m[0]) * 65536n + fdiv(B(cx) * 65536n * B(m[2]), B(W)), B(m[1]) * 65536n + fdiv(B(cy) * 65536n * B(m[3]), B(H)),
                         fdiv(Ux * B(m[2]), B(W)), fdiv(Uy * B(m[3]), B(H)), fdiv(Vx * B(m[2]), B(W)), fdiv(Vy * B(m[3]), B(H))] };
}
function terms(P, v) { const out = new Array(P); for (let i = 0; i < P; i++) out[i] = Number(fdiv(BigInt(2 * i + 1 - P) * v, BigInt(2 * P))); return out; }
function objOf(c, s) {
  if (s < 0 || s >= c.cs.length) throw new Error('mock addon: status -1: stream ' + s + ' is not reserved');
  const st = c.cs[s];
  if (!st) return [0, 0, 0, 0, 0];
  const v = new DataView(st.buffer, st.byteOffset);
  return [0, 1, 2, 3, 4].map(function (k) { return v.getFloat64(OBJ_OFFSET + 8 * k, true); });
}
/* the source's declared RGBA view: a packed frame at S[off ..] */
function viewOf(e) {
  const S = e.dev.buf, off = e.offset, w = e.SW, h = e.SH;
  if (e.format === DRAW_RGBA) return S.subarray(off, off + w * h * 4);
  const k = YUV[e.matrix || 0], cw = (w + 1) >> 1, ch = (h + 1) >> 1, cbase = off + w * h, out = new Uint8Array(w * h * 4);
  const clamp = function (v) { return v < 0 ? 0 : v > 255 ? 255 : v; };
  for (let y = 0; y < h; y++) for (let x = 0; x < w; x++) {
    const ci = (y >> 1) * cw + (x >> 1);
    const U = e.format === 0 ? S[cbase + 2 * ci] : S[cbase + ci], V = e.format === 0 ? S[cbase + 2 * ci + 1] : S[cbase + cw * ch + ci];
    const C = (S[off + y * w + x] - k[0]) * k[1], D = U - 128, E = V - 128, o = 4 * (y * w + x);
    out[o] = clamp((C + k[2] * E + 128) >> 8); out[o + 1] = clamp((C + k[3] * D + k[4] * E + 128) >> 8); out[o + 2] = clamp((C + k[5] * D + 128) >> 8); out[o + 3] = 255;
  }
  return out;
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
  const P = p.w, Q = p.h, pb = P * Q * 4, stride = ostride || pb, off = ooff || 0, n = entries.length;
  if (off + (n - 1) * stride + pb > out.buf.length) throw new RangeError('mock addon: output outside the device buffer');
  const plans = entries.map(function (e) { return plan(objOf(c, e.stream), c.w, c.h, e.mapping, p.margin, p.flags); });
  c.align = { n: n, records: new Int32Array(4 * n), terms: new Float64Array(6 * n) };
  entries.forEach(function (e, k) {
    const at = off + k * stride, pl = plans[k], D = out.buf;
    c.align.records.set([pl ? 1 : 0, e.stream, pl ? pl.a12 : 0, 0], 4 * k);
    D.fill(0, at, at + pb);
    if (!pl) return;
    c.align.terms.set(pl.t.map(Number), 6 * k);
    const V = viewOf(e), SW = e.SW, SH = e.SH;
    const cxs = terms(P, pl.t[2]), cys = terms(P, pl.t[3]), rxs = terms(Q, pl.t[4]), rys = terms(Q, pl.t[5]), Cx = Number(pl.t[0]) - 32768, Cy = Number(pl.t[1]) - 32768;
    for (let j = 0; j < Q; j++) for (let i = 0; i < P; i++) {
      const fx = Cx + cxs[i] + rxs[j], fy = Cy + cys[i] + rys[j]; /* below 2^52: exact */
      if (fx < -32768 || fy < -32768 || fx >= SW * 65536 - 32768 || fy >= SH * 65536 - 32768) continue;
      const xi = Math.floor(fx / 65536), yi = Math.floor(fy / 65536), tx = (fx - xi * 65536) >> 8, ty = (fy - yi * 65536) >> 8;
      const xa = Math.max(xi, 0), xb = Math.min(xi + 1, SW - 1), ya = Math.max(yi, 0), yb = Math.min(yi + 1, SH - 1);
      for (let ch = 0; ch < 4; ch++) {
        const top = V[4 * (ya * SW + xa) + ch] * (256 - tx) + V[4 * (ya * SW + xb) + ch] * tx, bot = V[4 * (yb * SW + xa) + ch] * (256 - tx) + V[4 * (yb * SW + xb) + ch] * tx;
        D[at + 4 * (j * P + i) + ch] = Math.floor((top * (256 - ty) + bot * ty + 32768) / 65536);
      }
    }
  });
}

const align = {
  ALIGN_EMPTY: 0, ALIGN_FACE: 1, ALIGN_SQUARE: 1,
  alignPairsDevice: function (c, pairs, prm, out, ostride, ooff, wait) {
    mock.calls.alignPairsDevice = (mock.calls.alignPairsDevice || 0) + 1; live(c);
    if (!(pairs instanceof Int32Array) || pairs.length < 2 || (pairs.length & 1)) throw new TypeError('mock addon: alignPairsDevice(ctx, Int32Array pairs[2n], ...)');
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
  alignSourcesDevice: function (c, streams, list, prm, out, ostride, ooff, wait) {
    mock.calls.alignSourcesDevice = (mock.calls.alignSourcesDevice || 0) + 1; live(c);
    if (!(streams instanceof Int32Array) || !Array.isArray(list) || list.length < 1 || streams.length !== list.length) throw new TypeError('mock addon: alignSourcesDevice(ctx, Int32Array streams[n], entries[n], ...)');
    const p = params(prm);
    const entries = list.map(function (e, i) {
      const whole = !e.rect || (e.rect[2] === 0 && e.rect[3] === 0);
      const m = whole ? [0, 0, e.width, e.height] : Array.from(e.rect);
      if (m[0] < 0 || m[1] < 0 || m[2] <= 0 || m[3] <= 0 || m[0] + m[2] > e.width || m[1] + m[3] > e.height) throw new Error('mock addon: status -1: entry ' + i + ': source rect must lie wholly inside the source frame');
      return { stream: streams[i], dev: e.dev, offset: e.offset || 0, SW: e.width, SH: e.height, format: e.format, matrix: e.matrix, mapping: m };
    });
    run(c, entries, p, out, ostride, ooff);
  },
  alignResult: function (c, n) {
    mock.calls.alignResult = (mock.calls.alignResult || 0) + 1; live(c);
    if (!c.align) throw new Error('mock addon: status -6: no align call to report on');
    if (n !== c.align.n) throw new Error('mock addon: status -6: n differs from the last align call');
    return { records: Int32Array.from(c.align.records), terms: Float64Array.from(c.align.terms) };
  }
};

mock.withAlign = function (on) {
  Object.keys(align).forEach(function (k) { if (on) mock[k] = align[k]; else delete mock[k]; });
  return mock;
};
module.exports = mock;
