'use strict';
/* tests/js/mock_addon_draw_list.js — TEST INFRASTRUCTURE: tests/js/mock_addon_yuv.js (left as it is) plus drawListDevice of csrc/ht_napi.cc:
 * every entry {dev, offset, width, height, format, matrix, rect} is ONE packed frame in a device buffer of its own and is drawn by the
 * mock's single-source draws (the declared conversion and the declared resampler of oracle/canvas_shim.js) onto frame i, so that the host
 * logic of ccv.DeviceBatch with opts.sources runs without a GPU.  The single-source draws are borrowed, not called by the facade: their
 * counters are put back, so that `calls` shows which entry point the FACADE took.  Needs withIngest(true) and withYuv(true).
 * `withDrawList(false)`: an addon that lacks the call. */
const path = require('path');
const mock = require(path.join(__dirname, 'mock_addon_yuv.js'));
const DRAW_RGBA = 16;

const list = {
  drawListDevice: function (c, entries, d, dstride, doff, wait) {
    mock.calls.drawListDevice = (mock.calls.drawListDevice || 0) + 1;
    if (!c || c.kind !== 'ctx' || c.destroyed) throw new TypeError('mock addon: expected a live context');
    if (!Array.isArray(entries) || entries.length < 1 || entries.length > 65535) throw new RangeError('mock addon: 1..65535 entries');
    if (!(c.w > 0 && c.h > 0)) throw new Error('mock addon: status -6: no geometry');
    const n = entries.length, fb = c.w * c.h * 4, boundForm = d === null || d === undefined, ds = dstride || fb, off = doff || 0;
    if (boundForm && n > c.maxBatch) throw new Error('mock addon: status -1: entry ' + c.maxBatch + ': more entries than the batch capacity');
    const target = boundForm ? { kind: 'dev', buf: new Uint8Array(n * fb) } : d;
    if (!boundForm && off + (n - 1) * ds + fb > d.buf.length) throw new RangeError('mock addon: destination outside the device buffer');
    const saved = Object.assign({}, mock.calls);
    try {
      entries.forEach(function (e, i) {
        if (!e || !e.dev) throw new TypeError('mock addon: an entry is {dev, offset, width, height, format, matrix, rect}');
        const rect = e.rect === undefined ? null : e.rect, at = (boundForm ? 0 : off) + i * (boundForm ? fb : ds);
        try {
          if (e.format === DRAW_RGBA) mock.drawFramesDevice(c, e.dev, e.offset || 0, 1, e.width, e.height, 0, 0, rect, target, at, 0, false);
          else mock.drawFramesYuvDevice(c, e.dev, e.offset || 0, 1, e.width, e.height, e.format, e.matrix || 0, 0, rect, target, at, 0, false);
        } catch (err) { err.message = 'entry ' + i + ': ' + err.message; throw err; }
      });
    } finally {
      Object.keys(mock.calls).forEach(function (k) { if (k in saved) mock.calls[k] = saved[k]; else delete mock.calls[k]; });
    }
    if (boundForm) { c.frames = target.buf; c.n = n; c.stride = fb; }
    if (wait) mock.calls.drawListDeviceWaited = (mock.calls.drawListDeviceWaited || 0) + 1;
  }
};

/* what a test needs to read a batch's frames back: the contexts and device buffers created since traceReset(), in creation order (a
 * ccv.DeviceBatch creates its contexts first, then its frame-set buffer, then the feeds' buffers) */
mock.trace = { ctxs: [], devs: [] };
mock.traceReset = function () { mock.trace.ctxs.length = 0; mock.trace.devs.length = 0; };
const baseCreate = mock.createContext, baseAlloc = mock.deviceAlloc;
mock.createContext = function () { const c = baseCreate.apply(this, arguments); mock.trace.ctxs.push(c); return c; };
mock.deviceAlloc = function () { const d = baseAlloc.apply(this, arguments); mock.trace.devs.push(d); return d; };

mock.withDrawList = function (on) {
  Object.keys(list).forEach(function (k) { if (on) mock[k] = list[k]; else delete mock[k]; });
  return mock;
};
module.exports = mock;
