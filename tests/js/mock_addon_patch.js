'use strict';
/* tests/js/mock_addon_patch.js — TEST INFRASTRUCTURE: tests/js/mock_addon_align.js (left as it is; it extends the same mock object) plus the
 * tensor entry points of csrc/ht_napi.cc — cropPairsTensorDevice, cropSourcesTensorDevice, alignPairsTensorDevice, alignSourcesTensorDevice —
 * so that ccv.DeviceBatch's opts.tensor runs without a GPU.  A tensor call IS the RGBA call of the same name (the mock's own, into a scratch
 * buffer: records and all) followed by the rule restated here: the source byte (gray: ccv.js:29 in binary64, round half to even), two
 * binary32 operations (Math.fround of a binary64 product / sum of binary32 operands is the correctly rounded binary32 result), the element
 * bits (binary16 and bfloat16 in integer arithmetic), the layout.  Needs withCrop and withAlign.  `withPatch(false)`: an addon without the calls. */
const path = require('path');
const mock = require(path.join(__dirname, 'mock_addon_align.js'));
const F32 = new Float32Array(1), U32 = new Uint32Array(F32.buffer);
function bitsOf(v) { F32[0] = v; return U32[0]; }
function roundHalfEven(v) { const f = Math.floor(v), d = v - f; return d > 0.5 ? f + 1 : d < 0.5 ? f : (f & 1 ? f + 1 : f); }
function gray(r, g, b) { const q = roundHalfEven(r * 0.3 + g * 0.59 + b * 0.11); return q < 0 ? 0 : q > 255 ? 255 : q; }
function f16Bits(v) {
  const u = bitsOf(v), sign = (u >>> 16) & 0x8000, a = u & 0x7fffffff;
  if (a >= 0x47800000) return sign | 0x7c00;
  if (a >= 0x38800000) { const r = a - 0x38000000, q = (r + 0xfff + ((r >>> 13) & 1)) >>> 13; return sign | (q > 0x7c00 ? 0x7c00 : q); }
  const e = a >>> 23;
  if (e < 102) return sign;
  const m = (a & 0x7fffff) | 0x800000, shift = 126 - e, q = m >>> shift, rem = m & ((1 << shift) - 1), half = 1 << (shift - 1);
  return sign | (q + ((rem > half || (rem === half && (q & 1))) ? 1 : 0));
}
function bf16Bits(v) { const u = bitsOf(v); return ((u + 0x7fff + ((u >>> 16) & 1)) >>> 16) & 0xffff; }
function format(f) {
  if (!f || typeof f !== 'object' || !Number.isInteger(f.dtype) || !Number.isInteger(f.layout) || !Number.isInteger(f.channels) || !(f.scale instanceof Float32Array) ||
      f.scale.length !== 3 || !(f.bias instanceof Float32Array) || f.bias.length !== 3) throw new TypeError('mock addon: format is {dtype, layout, channels, scale: Float32Array[3], bias: Float32Array[3]}');
  if (f.dtype < 0 || f.dtype > 2 || f.layout < 0 || f.layout > 1 || f.channels < 0 || f.channels > 2) throw new Error('mock addon: status -1: format: unknown dtype, layout or channels value');
  const C = f.channels === 2 ? 1 : 3;
  for (let c = 0; c < 3; c++) for (const v of [f.scale[c], f.bias[c]]) {
    const a = Math.abs(v);
    if (c >= C ? !Object.is(a, 0) : !(a === 0 || (a >= Math.pow(2, -64) && a <= Math.pow(2, 64)))) throw new Error('mock addon: status -1: format: scale / bias out of bounds');
  }
  return { C: C, esize: f.dtype === 0 ? 4 : 2 };
}
/* n RGBA patches of P x Q in rgba -> the tensor bytes in out.buf at ooff, stride apart */
function convert(rgba, n, P, Q, f, t, out, stride, ooff) {
  const pb = t.C * P * Q * t.esize;
  if (ooff + (n - 1) * stride + pb > out.buf.length) throw new RangeError('mock addon: output outside the device buffer');
  const view = new DataView(out.buf.buffer, out.buf.byteOffset);
  for (let k = 0; k < n; k++) for (let y = 0; y < Q; y++) for (let x = 0; x < P; x++) {
    const o = 4 * ((k * Q + y) * P + x), px = [rgba[o], rgba[o + 1], rgba[o + 2]];
    for (let c = 0; c < t.C; c++) {
      const b = f.channels === 2 ? gray(px[0], px[1], px[2]) : f.channels === 1 ? px[2 - c] : px[c];
      const v = Math.fround(Math.fround(b * f.scale[c]) + f.bias[c]);
      const el = f.layout === 0 ? c * P * Q + y * P + x : (y * P + x) * t.C + c, at = ooff + k * stride + el * t.esize;
      if (f.dtype === 0) view.setUint32(at, bitsOf(v), true);
      else view.setUint16(at, f.dtype === 1 ? f16Bits(v) : bf16Bits(v), true);
    }
  }
}
function tensorCall(name, rgbaName, listAt) {
  return function () {
    const a = Array.prototype.slice.call(arguments);
    mock.calls[name] = (mock.calls[name] || 0) + 1;
    const prm = a[listAt + 1], f = a[listAt + 2], out = a[listAt + 3], ostride = a[listAt + 4], ooff = a[listAt + 5] || 0;
    const t = format(f);
    if (!out || out.kind !== 'dev' || !out.buf) throw new TypeError('mock addon: expected a live device buffer');
    const n = listAt === 1 ? a[1].length >> 1 : a[2].length, P = prm[0], Q = prm[1], pb = t.C * P * Q * t.esize;
    if (ostride && (ostride % 4 || ostride < pb)) throw new Error('mock addon: status -1: output stride smaller than a patch or not a multiple of 4');
    const scratch = { kind: 'dev', buf: new Uint8Array(n * P * Q * 4) };
    const before = mock.calls[rgbaName] || 0;
    mock[rgbaName].apply(mock, a.slice(0, listAt + 2).concat([scratch, 0, 0, false]));
    mock.calls[rgbaName] = before; /* the RGBA entry point was not called by the facade */
    convert(scratch.buf, n, P, Q, f, t, out, ostride || ((pb + 3) & ~3), ooff);
  };
}
const patch = {
  PATCH_F32: 0, PATCH_F16: 1, PATCH_BF16: 2, PATCH_CHW: 0, PATCH_HWC: 1, PATCH_RGB: 0, PATCH_BGR: 1, PATCH_GRAY: 2,
  cropPairsTensorDevice: tensorCall('cropPairsTensorDevice', 'cropPairsDevice', 1),
  cropSourcesTensorDevice: tensorCall('cropSourcesTensorDevice', 'cropSourcesDevice', 2),
  alignPairsTensorDevice: tensorCall('alignPairsTensorDevice', 'alignPairsDevice', 1),
  alignSourcesTensorDevice: tensorCall('alignSourcesTensorDevice', 'alignSourcesDevice', 2)
};
mock.withPatch = function (on) {
  Object.keys(patch).forEach(function (k) { if (on) mock[k] = patch[k]; else delete mock[k]; });
  return mock;
};
module.exports = mock;
